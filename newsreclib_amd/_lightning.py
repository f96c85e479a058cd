"""Base class for the drop-in module: ``lightning.LightningModule`` when Lightning is installed
(the reference's runtime, ``abstract_recommender.py:17``), else a minimal stand-in with the members
the module itself uses (``save_hyperparameters``/``hparams``, ``log``/``log_dict``, ``device``).
Lightning is not installed in the build image, so the stand-in is what the tests exercise."""
import inspect
from types import SimpleNamespace

import torch
import torch.nn as nn

try:  # pragma: no cover - depends on the environment
    from lightning import LightningModule as _Base
    HAVE_LIGHTNING = True
except Exception:  # noqa: BLE001
    try:  # pragma: no cover
        from pytorch_lightning import LightningModule as _Base
        HAVE_LIGHTNING = True
    except Exception:  # noqa: BLE001
        _Base = None
        HAVE_LIGHTNING = False


class _HParams(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def keys(self):
        return self.__dict__.keys()


class _MiniLightningModule(nn.Module):
    def __init__(self):
        super().__init__()
        self._hparams = _HParams()
        self.logged = {}

    def save_hyperparameters(self, *args, logger=True, ignore=(), **kwargs):
        frame = inspect.currentframe().f_back
        # walk up to the outermost __init__ of this object so subclass kwargs are captured
        init_args = {}
        while frame is not None:
            local = frame.f_locals
            if local.get("self") is self and frame.f_code.co_name == "__init__":
                for k, v in local.items():
                    if k not in ("self", "__class__", "args", "kwargs") and not k.startswith("_") \
                            and k not in ignore:
                        init_args.setdefault(k, v)
                for k, v in local.get("kwargs", {}).items():
                    init_args.setdefault(k, v)
            frame = frame.f_back
        self._hparams = _HParams(**init_args)

    @property
    def hparams(self):
        return self._hparams

    @property
    def device(self):
        try:
            return next(self.parameters()).device
        except StopIteration:
            return torch.device("cpu")

    def log(self, name, value, **kwargs):
        self.logged[name] = value

    def log_dict(self, d, **kwargs):
        self.logged.update(dict(d))

    # -- manual optimization (LightningModule.optimizers / toggle_optimizer / untoggle_optimizer / manual_backward): what a module
    #    with several optimizers drives from its own training_step ------------------------------------------------------------
    automatic_optimization = True

    def optimizers(self):
        """The optimizers of the module as a list: the ones a trainer installed (``install_optimizers``), else built ONCE from
        ``configure_optimizers()`` and kept."""
        opts = self.__dict__.get("_optimizers")
        if opts is None:
            cfg = self.configure_optimizers()
            if isinstance(cfg, dict):
                cfg = [cfg["optimizer"]]
            elif not isinstance(cfg, (list, tuple)):
                cfg = [cfg]
            opts = [c["optimizer"] if isinstance(c, dict) else c for c in cfg]
            self.__dict__["_optimizers"] = opts
        return opts

    def install_optimizers(self, optimizers) -> None:
        """Not a Lightning member: how a trainer of this library (``trainer.SentiDebiasTrainer``) hands the module the
        optimizers it built, the part Lightning's own ``Trainer`` plays for ``optimizers()``."""
        self.__dict__["_optimizers"] = list(optimizers)

    @staticmethod
    def _owned_params(optimizer):
        return [p for group in optimizer.param_groups for p in group["params"]]

    def toggle_optimizer(self, optimizer) -> None:
        """Only the parameters ``optimizer`` owns keep their ``requires_grad``; every parameter of every other optimizer is
        switched off until ``untoggle_optimizer`` (a parameter that was already frozen stays frozen throughout).  One toggle at
        a time, as in Lightning: toggling again before ``untoggle_optimizer`` is a misuse and raises, since the second call
        would save the switched-off flags over the real ones."""
        if self.__dict__.get("_toggled_flags"):
            raise RuntimeError("toggle_optimizer: another optimizer is still toggled; call untoggle_optimizer first")
        saved = {}
        for opt in self.optimizers():
            for p in self._owned_params(opt):
                if p not in saved:
                    saved[p] = p.requires_grad
                    p.requires_grad = False
        for p in self._owned_params(optimizer):
            p.requires_grad = saved[p]
        self.__dict__["_toggled_flags"] = saved

    def untoggle_optimizer(self, optimizer) -> None:
        saved = self.__dict__.get("_toggled_flags") or {}
        for p, flag in saved.items():
            p.requires_grad = flag
        self.__dict__["_toggled_flags"] = {}

    def manual_backward(self, loss, *args, **kwargs) -> None:
        loss.backward(*args, **kwargs)


LightningModuleBase = _Base if HAVE_LIGHTNING else _MiniLightningModule
