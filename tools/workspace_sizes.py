#!/usr/bin/env python3
"""Prints, as JSON, the value of every exported ``*_workspace_bytes`` function of a built library over a fixed grid of shapes.

    python tools/workspace_sizes.py [path/to/libnewsreclib_amd.so] > tests/data/workspace_sizes.json

The size functions touch no device.  Run it with no NRL_* variable set: some regions depend on the kernel switches.
tests/test_workspace_host.py compares the committed table with the built library, so a change of any workspace layout shows
up as a diff of that file; a pull request that changes a layout on purpose regenerates it with this tool.
"""
from __future__ import annotations

import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from newsreclib_amd import _lib  # noqa: E402  (ctypes signatures only: nothing is loaded by the import)

PLACEHOLDER = 256          # a non-null, aligned "pointer" for parameter structs whose fields are only checked, never read


def _npa_query_params(user_dim, text_q, news_q, filters, news_head):
    p = _lib.NrlNpaQueryParams()
    if news_head:
        p.news_proj_weight = PLACEHOLDER
    p.num_users, p.user_dim, p.text_query_dim, p.news_query_dim, p.num_filters = 1000, user_dim, text_q, news_q, filters
    return p


def _dkn_params(windows, word_dim, entity_dim, filters, context):
    p = _lib.NrlDknParams()
    p.word_table = p.entity_table = p.transform_matrix = p.transform_bias = PLACEHOLDER
    if context:
        p.context_table = PLACEHOLDER
    for i, w in enumerate(windows):
        p.conv_image[i] = p.conv_bias[i] = PLACEHOLDER
        p.windows[i] = w
    p.num_windows, p.word_dim, p.entity_dim, p.num_filters = len(windows), word_dim, entity_dim, filters
    return p


def grid() -> dict[str, list[tuple]]:
    """function name -> argument tuples.  Every conditional region of every layout is reached by some tuple."""
    g: dict[str, list[tuple]] = {}
    # the shared block: the fused news path (padded planes; M % 32 zero and non-zero), no padding at D = 64, the user shape
    g["nrl_news_encoder_workspace_bytes"] = ([(n, 30, 300, 15, 200) for n in (0, 1, 7, 16, 33, 70)] +
                                             [(n, 30, 64, 4, 200) for n in (1, 7, 33)] +
                                             [(7, 50, 300, 15, 200), (7, 64, 300, 15, 200), (5, 30, 320, 16, 64), (4096, 30, 300, 15, 200)])
    g["nrl_user_encoder_workspace_bytes"] = [(b, 50, 300, 15, 200) for b in (0, 1, 3, 130)] + [(3, 50, 64, 4, 200), (130, 35, 400, 20, 200)]
    g["nrl_news_encoder_fwd_table_workspace_bytes"] = [(0, 30, 15), (1, 30, 15), (7, 30, 15), (33, 20, 15), (4096, 30, 15), (5, 30, 0)]
    cnn = list(itertools.product((1, 7, 33), (30,), (300,), (300, 400), (1, 3, 5), (200, 224, 228)))
    cnn += [(0, 30, 300, 300, 3, 200), (7, 63, 300, 300, 3, 200), (7, 64, 300, 300, 3, 200), (7, 20, 100, 320, 3, 200),
            (7, 30, 300, 304, 3, 200), (7, 30, 300, 316, 3, 200), (4096, 30, 300, 300, 3, 200), (4096, 30, 300, 400, 3, 200)]
    g["nrl_cnn_encoder_workspace_bytes"] = cnn
    g["nrl_cnn_mhsa_encoder_workspace_bytes"] = [(n, L, D, F, W, heads, Q) for (n, L, D, F, W, Q) in cnn if F % 20 == 0
                                                 for heads in ((20, 15) if F == 300 else (20,))]
    npa = [(n, 30, 300, F, W) for n in (0, 1, 7, 33, 4096) for F in (300, 400) for W in (1, 3, 5)] + [(7, 64, 300, 300, 3)]
    g["nrl_npa_encoder_workspace_bytes"] = npa
    g["nrl_npa_conv_features_workspace_bytes"] = npa
    g["nrl_npa_user_queries_workspace_bytes"] = [(_npa_query_params(u, tq, nq, f, nh), b)
                                                 for (u, tq, nq, f, nh) in ((50, 200, 200, 400, True), (50, 200, 300, 400, True),
                                                                            (50, 200, 300, 400, False), (4, 4, 4, 4, False))
                                                 for b in (0, 1, 3, 130)]
    g["nrl_dkn_encoder_workspace_bytes"] = [(_dkn_params(w, wd, ed, f, ctx), n, L)
                                            for (w, wd, ed, f, ctx) in (((1,), 4, 4, 4, False), ((1, 2, 3, 4), 100, 100, 100, True),
                                                                        ((2, 3), 300, 100, 52, False), ((3,), 300, 100, 100, True))
                                            for (n, L) in ((0, 10), (1, 4), (7, 10), (33, 30), (2048, 30))]
    g["nrl_dkn_click_workspace_bytes"] = [(0, 5, 400, 16), (1, 1, 1, 1), (3, 5, 400, 16), (130, 37, 1024, 64), (4, 0, 8, 4)]
    g["nrl_caum_score_workspace_bytes"] = [(0, 5, 50, 100), (1, 1, 1, 1), (3, 5, 50, 100), (130, 37, 50, 256), (2, 5, 8192, 4)]
    g["nrl_miner_wgrad_workspace_bytes"] = [(0, 32, 256), (1, 4, 4), (3, 32, 256), (6500, 32, 256), (1000000, 200, 768)]
    g["nrl_miner_categ_bias_workspace_bytes"] = [(1, 1, 1, 4), (3, 7, 5, 100), (3, 8, 12, 100), (130, 6500, 650, 100), (2, 3, 3, 6)]
    g["nrl_miner_poly_workspace_bytes"] = [(0, 32, 200), (1, 1, 4), (3, 32, 200), (130, 32, 200)]
    g["nrl_supcon_embed_workspace_bytes"] = [(0, 8), (1, 4), (3, 8), (7, 400), (512, 400), (1024, 400), (1025, 400), (4096, 400), (8, 0)]
    g["nrl_impression_metrics_workspace_bytes"] = [(0, 1, 0, 0), (100, 8, 0, 2), (37, 3, 1, 2), (100000, 4097, 2, 4), (5, 0, 0, 2), (5, 2, 3, 2)]
    g["nrl_topk_scores_workspace_bytes"] = [(0, 100, 8, 5, 0), (1, 1, 4, 1, 0), (4, 100, 8, 5, 0), (3, 1000, 300, 128, 7), (130, 63, 4, 5, 2),
                                            (512, 65536, 400, 10, 0), (512, 65536, 400, 10, 8), (4, 100, 6, 5, 0), (4, 0, 8, 5, 0)]
    g["nrl_sort_positions_workspace_bytes"] = [(0, 1), (0, 0), (1, 1), (210, 500), (100000, 1 << 20), (65, 1025)]
    g["nrl_gru_workspace_bytes"] = [(1, 1, 4, 4), (3, 50, 400, 400), (130, 50, 400, 400), (3, 7, 300, 100)]
    g["nrl_additive_attention_workspace_bytes"] = [(0, 50, 400, 200), (1, 1, 4, 4), (3, 50, 400, 200), (130, 50, 400, 200), (7, 30, 300, 228)]
    g["nrl_mha_workspace_bytes"] = [(0, 3, 400, 20), (1, 1, 16, 1), (50, 3, 400, 20), (50, 130, 400, 20), (7, 3, 64, 4)]
    g["nrl_linear_act_workspace_bytes"] = [(0, 200, 400), (1, 4, 4), (3, 200, 400), (6500, 400, 300), (7, 228, 300)]
    g["nrl_linear_workspace_bytes"] = [(4, 4), (200, 400), (256, 768), (768, 3072), (3072, 768), (300, 300)]
    g["nrl_linear3_workspace_bytes"] = [(256, 256), (768, 768), (256, 1024), (1024, 256)]
    return g


def _plain(arg):
    """A JSON-able description of one argument (parameter structs: their integer fields and which pointers are set)."""
    if isinstance(arg, ctypes.Structure):
        out = {}
        for name, _ in arg._fields_:
            v = getattr(arg, name)
            out[name] = [x or 0 for x in v] if isinstance(v, ctypes.Array) else (v or 0)
        return out
    return arg


def measure(lib_path: str) -> dict:
    lib = ctypes.CDLL(lib_path)
    names = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    g = grid()
    missing = sorted(set(names) ^ set(g))
    if missing:
        raise SystemExit(f"the grid and the declared *_workspace_bytes functions differ: {missing}")
    table = {}
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        rows = []
        for args in g[name]:
            call = [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args]
            rows.append({"args": [_plain(a) for a in args], "bytes": int(fn(*call))})
        table[name] = rows
    return table


def main() -> None:
    path = sys.argv[1] if len(sys.argv) > 1 else _lib.LIB_PATH
    json.dump(measure(path), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
