"""newsreclib_amd -- MI355X (gfx950) native NRMS hot path behind NewsRecLib's module interfaces.

Public surface (mirrors the reference's operator API for this path):

* ``newsreclib_amd.nrms_module.NRMSModule``  -- drop-in ``model._target_``
* ``newsreclib_amd.news_encoder.{MHSAAddAtt, NewsEncoder}``, ``user_encoder.UserEncoder``,
  ``click_predictor.DotProduct`` -- the sub-module interfaces
* ``newsreclib_amd.trainer.NRMSTrainer`` -- flat-buffer train step with RCCL data parallelism
* ``CRModule``, ``AModule``, ``MANNERModule`` (MANNeR: ``manner_cr_module`` / ``manner_a_module`` / ``manner_module``), importable from
  the package itself (resolved on first use, so importing the package stays free of torch)
* the C ABI itself: ``include/newsreclib_amd.h`` / ``newsreclib_amd/libnewsreclib_amd.so``
"""
__version__ = "0.1.0"

_LAZY = {"CRModule": "manner_cr_module", "AModule": "manner_a_module", "MANNERModule": "manner_module"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
