"""Guard bands around every native workspace: ``ops.workspace`` is replaced by an allocator that puts 4096 bytes of 0xA5 in
front of and behind the requested bytes and hands out the view between them (its offset of 4096 keeps the 256-byte alignment).
Each family runs one forward and one backward at the smallest case its own GPU test builds; afterwards every guard byte must
be intact, i.e. no kernel wrote outside the bytes its ``*_workspace_bytes`` function asked for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5


class Guards:
    def __init__(self):
        self.outer = []                     # (buffer, requested bytes): kept alive until the check

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 256)
        buf = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device=device)
        buf[:GUARD] = FILL
        buf[GUARD + n:] = FILL
        self.outer.append((buf, n))
        inner = buf[GUARD:GUARD + n]
        assert inner.data_ptr() % 256 == 0 and inner.numel() == n
        return inner

    def check(self):
        torch.cuda.synchronize()
        assert self.outer, "no workspace was requested through ops.workspace"
        bad = torch.stack([(b[:GUARD] != FILL).sum() + (b[GUARD + n:] != FILL).sum() for b, n in self.outer]).cpu().tolist()
        assert not any(bad), [(i, self.outer[i][1], c) for i, c in enumerate(bad) if c]


@pytest.fixture
def guards(monkeypatch):
    from newsreclib_amd import ops
    g = Guards()
    monkeypatch.setattr(ops, "workspace", g)
    return g


def _t(rng, *shape, scale=1.0, grad=True):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).cuda().requires_grad_(grad)


def _block_params(rng, D, Q):
    return [_t(rng, 3 * D, D, scale=D ** -0.5), _t(rng, 3 * D, scale=0.05), _t(rng, D, D, scale=D ** -0.5), _t(rng, D, scale=0.05),
            _t(rng, Q, D, scale=D ** -0.5), _t(rng, Q, scale=0.05), _t(rng, Q, scale=0.1)]


def _offsets(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).cuda()


@pytest.mark.parametrize("engine", ["f32", "bf16x3"])
@pytest.mark.parametrize("n_news", [7, 33])
def test_fused_news_encoder(n_news, engine, guards):
    from newsreclib_amd import _lib, ops
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(engine)
    try:
        rng = np.random.default_rng(n_news)
        V, L, D, heads, Q = 50, 30, 300, 15, 200
        emb = _t(rng, V, D, scale=0.3)
        ids = torch.from_numpy(rng.integers(0, V, (n_news, L))).cuda()
        ids[:, 20:] = 0
        out = ops.NewsEncoderFn.apply(ids, emb, *_block_params(rng, D, Q), heads, 0.2, 11, 2, None)
        out.backward(_t(rng, n_news, D, grad=False))
        guards.check()
    finally:
        _lib.set_gemm_engine(prev)


def test_nrms_user_encoder(guards):
    from newsreclib_amd import ops
    rng = np.random.default_rng(3)
    B, H, D, heads, Q = 3, 50, 300, 15, 200
    hist = _t(rng, B, H, D, scale=0.5)
    out = ops.UserEncoderFn.apply(hist, *_block_params(rng, D, Q), heads, None, 0.1, 99)
    out.backward(_t(rng, B, D, grad=False))
    guards.check()


@pytest.mark.parametrize("shape", [(3, 4, 16, 16, 1, 8), (5, 30, 300, 300, 3, 200)])
def test_lstur_cnn_encoder(shape, guards):
    from newsreclib_amd.ops_lstur import CnnEncoderFn
    N, L, D, F, W, Q = shape
    rng = np.random.default_rng(N * 7 + L)
    V = 50
    params = [_t(rng, V, D, scale=0.3), _t(rng, F, 1, W, D, scale=(W * D) ** -0.5), _t(rng, F, scale=0.05),
              _t(rng, Q, F, scale=F ** -0.5), _t(rng, Q, scale=0.05), _t(rng, Q, scale=0.1)]
    ids = torch.from_numpy(rng.integers(0, V, (N, L))).cuda()
    ids[:, L - 2:] = 0
    out = CnnEncoderFn.apply(ids, *params, 0.2, 11, 2, None, None)
    out.backward(_t(rng, N, F, grad=False))
    guards.check()


def test_lstur_gru(guards):
    from newsreclib_amd.ops_lstur import GruFn
    B, T, Din, Hd = 3, 4, 16, 8
    rng = np.random.default_rng(B + T)
    hist, h0 = _t(rng, B, T, Din, scale=0.5), _t(rng, B, Hd, scale=0.5)
    lengths = torch.tensor([T, 1, 2]).cuda()
    params = [_t(rng, 3 * Hd, Din, scale=Din ** -0.5), _t(rng, 3 * Hd, Hd, scale=Hd ** -0.5), _t(rng, 3 * Hd, scale=0.05),
              _t(rng, 3 * Hd, scale=0.05)]
    out = GruFn.apply(hist, lengths, h0, *params, None)
    out.backward(_t(rng, B, Hd, grad=False))
    guards.check()


def test_cnn_mhsa_encoder(guards):
    """The composition CNN + MHSA block on one arena (CenNewsRec's text encoder)."""
    from newsreclib_amd.ops_lstur import CnnMhsaEncoderFn
    N, L, D, F, W, heads, Q = 3, 6, 16, 32, 3, 2, 8
    rng = np.random.default_rng(17)
    V = 50
    ids = torch.from_numpy(rng.integers(0, V, (N, L))).cuda()
    out = CnnMhsaEncoderFn.apply(ids, _t(rng, V, D, scale=0.3), _t(rng, F, 1, W, D, scale=(W * D) ** -0.5), _t(rng, F, scale=0.05),
                                 *_block_params(rng, F, Q), heads, 0.2, 11, 2, None)
    out.backward(_t(rng, N, F, grad=False))
    guards.check()


def test_additive_attention(guards):
    from newsreclib_amd.ops_blocks import AdditiveAttentionFn
    rng = np.random.default_rng(5)
    G, S, D, Q = 3, 7, 64, 20
    out = AdditiveAttentionFn.apply(_t(rng, G, S, D, scale=0.5), _t(rng, Q, D, scale=D ** -0.5), _t(rng, Q, scale=0.05),
                                    _t(rng, Q, scale=0.1), None)
    out.backward(_t(rng, G, D, grad=False))
    guards.check()


def test_mha(guards):
    from newsreclib_amd.ops_blocks import MhaFn
    S, Bt, D, heads = 45, 3, 32, 2
    rng = np.random.default_rng(S + D)
    out = MhaFn.apply(_t(rng, S, Bt, D, scale=0.5), _t(rng, 3 * D, D, scale=D ** -0.5), _t(rng, 3 * D, scale=0.05),
                      _t(rng, D, D, scale=D ** -0.5), _t(rng, D, scale=0.05), heads, None, None)
    out.backward(_t(rng, S, Bt, D, grad=False))
    guards.check()


@pytest.mark.parametrize("act", ["none", "tanh"])
def test_linear_act(act, guards):
    from newsreclib_amd.ops_blocks import LinearActFn
    M, N, K = 3, 8, 4
    rng = np.random.default_rng(M + N)
    out = LinearActFn.apply(_t(rng, M, K), _t(rng, N, K, scale=K ** -0.5), _t(rng, N, scale=0.1), act, None)
    out.backward(_t(rng, M, N, grad=False))
    guards.check()


def test_npa_encoder_and_queries(guards):
    from newsreclib_amd import ops_npa
    from tests import sweep_inputs as S
    case, inp = S.NPA_ENCODER_CASES[0], S.cached_inputs("npa_encoder", 0)
    leaves = {k: inp[k].cuda().requires_grad_(True) for k in ("emb", "w", "b", "queries")}
    w_img = leaves["w"].permute(0, 2, 1).contiguous().unsqueeze(1)
    out = ops_npa.NpaEncoderFn.apply(inp["ids"].cuda(), leaves["emb"], w_img, leaves["b"], leaves["queries"], inp["owner"].cuda(),
                                     inp["offsets"].cuda(), case["p"], S.DROP_SEED, ops_npa.ENCODER_STREAM0, None)
    out.backward(inp["d_out"].cuda())
    ops_npa.npa_conv_features(inp["ids"].cuda(), inp["emb"].cuda(), inp["w"].cuda(), inp["b"].cuda())
    case, inp = S.NPA_QUERY_CASES[0], S.cached_inputs("npa_query", 0)
    args = [inp[k].cuda().requires_grad_(True) if k in inp else None for k in S.QUERY_KEYS]
    text, news = ops_npa.NpaUserQueriesFn.apply(inp["user_idx"].cuda(), *args, case["p"], S.DROP_SEED, ops_npa.QUERY_STREAM0, None)
    torch.autograd.backward([text, news], [inp["d_text"].cuda(), inp["d_news"].cuda()])
    guards.check()


def test_dkn_encoder_and_click(guards):
    from newsreclib_amd import ops_dkn
    from tests import dkn_oracle as DO
    from tests import sweep_inputs as S
    case, inp = S.DKN_ENCODER_CASES[0], S.cached_inputs("dkn_encoder", 0)
    leaves = {k: v.cuda().requires_grad_(True) for k, v in inp["params"].items()}
    windows = case["windows"]
    convs = [leaves[DO.conv_key(x, what)] for x in windows for what in ("weight", "bias")]
    images = [leaves[DO.conv_key(x, "weight")].detach().permute(0, 2, 1, 3).contiguous() for x in windows]
    out = ops_dkn.DknEncoderFn.apply(inp["ids"].cuda(), inp["ents"].cuda(), None, tuple(windows), images, None, leaves[DO.WORD],
                                     leaves[DO.ENT], leaves.get(DO.CTX), leaves[DO.TM], leaves[DO.TB], *convs)
    out.backward(torch.ones_like(out))
    case, inp = S.DKN_CLICK_CASES[0], S.cached_inputs("dkn_click", 0)
    keys = ["hist", "cand"] + list(S.CLICK_KEYS)
    leaves = {k: inp[k].cuda().requires_grad_(True) for k in keys}
    scores = ops_dkn.DknClickFn.apply(leaves["hist"], inp["hist_offsets"].cuda(), max(case["hist"]), leaves["cand"],
                                      inp["cand_offsets"].cuda(), max(case["cand"]), *[leaves[k] for k in S.CLICK_KEYS])
    scores.backward(inp["d_scores"].cuda())
    guards.check()


def test_caum_score(guards):
    from newsreclib_amd import ops_caum
    rng = np.random.default_rng(9)
    B, C, H, N2, U = 2, 3, 5, 8, 16
    R = B * C * H
    scores = ops_caum.ScoreFn.apply(_t(rng, R, N2, scale=0.5), _t(rng, 1, N2, scale=0.3), _t(rng, 1, scale=0.1), _t(rng, R, U, scale=0.5),
                                    _t(rng, B * C, U, scale=0.5), _offsets([3, 2]), B, C, 0, None)
    scores.backward(_t(rng, B, C, grad=False))
    guards.check()


def test_miner_wgrad_category_bias_and_poly(guards):
    from newsreclib_amd import ops_miner
    rng = np.random.default_rng(5)
    sizes, cands = [5, 3, 1], [2, 4, 1]
    B, D, Cd, K, Dc = 3, 64, 24, 8, 12
    nh, nc = sum(sizes), sum(cands)
    hist_off, cand_off = _offsets(sizes), _offsets(cands)
    bh = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).cuda()
    bc = torch.repeat_interleave(torch.arange(B), torch.tensor(cands)).cuda()
    bias = ops_miner.CategBiasFn.apply(_t(rng, nh, Dc), _t(rng, nc, Dc), bh, bc, hist_off, cand_off, B)
    E, codes = _t(rng, nh, D, scale=0.5), _t(rng, K, Cd, scale=0.5)
    P = ops_miner.BiasFreeLinearFn.apply(E, _t(rng, Cd, D, scale=0.2), "tanh")         # (weight gradient: nrl_miner_wgrad)
    uv = ops_miner.PolyFn.apply(E, P, codes, bias, hist_off, B, max(sizes))
    z = ops_miner.BiasFreeLinearFn.apply(uv.reshape(B * K, D), _t(rng, D, D, scale=D ** -0.5), None)
    (uv.sum() + z.sum()).backward()
    guards.check()


@pytest.mark.parametrize("n", [7, 130])          # one column chunk of 128 anchors, and two (the per-chunk region exists)
def test_supcon_embed(n, guards):
    from newsreclib_amd.ops_manner import supcon_embed_fwd_bwd
    rng = np.random.default_rng(n)
    E = torch.nn.functional.normalize(_t(rng, n, 16, grad=False), dim=1).contiguous()
    supcon_embed_fwd_bwd(E, torch.from_numpy(rng.integers(0, 4, n)).cuda(), 0.9)
    guards.check()


def test_impression_metrics_topk_and_sort_positions(guards):
    from newsreclib_amd import ops
    rng = np.random.default_rng(4)
    sizes = [5, 1, 9]
    preds = _t(rng, sum(sizes), grad=False)
    targets = torch.zeros(sum(sizes), device="cuda")
    targets[[0, 5, 8]] = 1.0
    ops.impression_metrics(preds, targets, _offsets(sizes), (5, 10))
    ops.topk_scores(_t(rng, 3, 8, grad=False), _t(rng, 100, 8, grad=False), 5)
    ops.sort_positions(torch.from_numpy(rng.integers(0, 23, (7, 30))).cuda(), 23)
    guards.check()
