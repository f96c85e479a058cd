"""Full-catalogue rank of held-out clicks under the MINER, DKN and NPA scorers (``nrl_catalogue_interest_ranks`` /
``ops.catalogue_interest_ranks`` / ``NewsVectorCache.rank_clicks_interests``, ``nrl_catalogue_relu_ranks`` /
``ops.catalogue_relu_ranks`` / ``NewsVectorCache.rank_clicks_dnn`` and ``nrl_catalogue_pooled_ranks`` /
``ops.catalogue_pooled_ranks`` / ``NpaFeatureCache.rank_clicks_pooled``, and ``evaluate_full_rank`` over all three).

Expected values come from ``tests/catalogue_rank_scorers_ref.py`` under ``tests/catalogue_ref.py`` (CPU, float64).  Integer-valued inputs in [-4, 4] (NPA: the exact
family of ``topk_npa_ref``) make every fp32 score exact (``test_catalogue_rank_scorers_host.py`` asserts what that rests on), so those cases compare with ``torch.equal``,
ties included.  Against ``ops.topk_*`` the check is a derived condition with no tolerance: ``rank = r <= k`` exactly when slot
``r - 1`` of the list is the target, with the list's score bits.  Against float64 a rank must lie in the interval the derived
bounds of the two rows leave open (``catalogue_ref.rank_intervals``); the host tier asserts that interval is one rank wide for at least 90 % of
the targets used here."""
import pytest
import torch

from tests import builders
from tests import catalogue_ref as C
from tests import catalogue_rank_scorers_ref as R

pytestmark = pytest.mark.gpu

E_EXCLUDE, E_OFFSETS, E_NAN, E_TARGETS, E_TARGET_ROW = 1, 2, 4, 16, 32
NEG_INF = float("-inf")
_F32 = {}                                                  # results recorded under the f32 engine, compared under bf16x3


@pytest.fixture(autouse=True, params=["f32", "bf16x3"])
def engine(request):
    from newsreclib_amd import _lib
    prev = _lib.get_gemm_engine()
    _lib.set_gemm_engine(request.param)
    yield request.param
    _lib.set_gemm_engine(prev)


# ---- the three families behind one face ----------------------------------------------------------------------------------------------
# a case: {"kind", "user": per-user tensors (first dimension B), "shared": the table side, "mode" (MINER)}
def _miner(E, G, T, mode):
    return {"kind": "miner", "user": (E, G), "shared": (T,), "mode": mode}


def _dkn(q, proj, w2, b2):
    return {"kind": "dkn", "user": (q,), "shared": (proj, w2, b2), "mode": None}


def _npa(q, user, feat):
    return {"kind": "npa", "user": (q, user), "shared": (feat,), "mode": None}


def _int_case(kind, seed, shape, mode=None):
    if kind == "npa":
        return _npa(*R.NR.exact_case(seed, *shape)[:3])
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randint(-4, 5, s, generator=g).float()  # noqa: E731
    if kind == "miner":
        B, K, V, D = shape
        return _miner(r(B, K, D), r(B, K, D), r(V, D), mode)
    B, V, Hd = shape
    return _dkn(r(B, Hd), r(V, Hd), torch.randint(-3, 4, (Hd,), generator=g).float(), torch.tensor([2.0]))


def _real_case(kind, seed, shape, mode=None):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if kind == "miner":
        B, K, V, D = shape
        return _miner(r(B, K, D), r(B, K, D), r(V, D), mode)
    if kind == "npa":                                            # the real family of topk_npa_ref
        B, V, L, F = shape
        return _npa(torch.tanh(0.25 * r(B, F)), r(B, F) / F ** 0.5, torch.relu(r(V, L, F)))
    B, V, Hd = shape
    return _dkn(r(B, Hd), r(V, Hd), r(Hd) / Hd ** 0.5, 0.1 * r(1))


def _sizes(c):
    return c["user"][0].shape[0], c["shared"][0].shape[0]


def _take(c, sel):
    return dict(c, user=tuple(t[sel] for t in c["user"]))


def _with(c, user=None, shared=None):
    return dict(c, user=user if user is not None else c["user"], shared=shared if shared is not None else c["shared"])


def _scores64(c):
    if c["kind"] == "miner":
        return R.interest_scores64(c["user"][0], c["shared"][0], c["mode"], c["user"][1])[0]
    if c["kind"] == "npa":
        return R.NR.scores64(c["user"][0], c["user"][1], c["shared"][0])[0]
    return R.DR.relu_scores64(c["user"][0], *c["shared"])


def _call(c, ti, to, ei=None, eo=None, elig=None, slices=0):
    """The family's ``ops`` rank entry on device tensors -> its device outputs."""
    from newsreclib_amd import ops
    if c["kind"] == "miner":
        E, G = c["user"]
        return ops.catalogue_interest_ranks(E.cuda(), c["shared"][0].cuda(), ti, to, c["mode"],
                                            G.cuda() if c["mode"] == "weighted" else None, ei, eo, elig, slices)
    if c["kind"] == "npa":
        return ops.catalogue_pooled_ranks(c["user"][0].cuda(), c["user"][1].cuda(), c["shared"][0].cuda(), ti, to, ei, eo, elig, slices)
    proj, w2, b2 = c["shared"]
    return ops.catalogue_relu_ranks(c["user"][0].cuda(), proj.cuda(), w2.cuda(), b2.cuda(), ti, to, ei, eo, elig, slices)


def _topk(c, k, ei=None, eo=None, elig=None):
    from newsreclib_amd import ops
    if c["kind"] == "miner":
        E, G = c["user"]
        return ops.topk_interest_scores(E.cuda(), c["shared"][0].cuda(), k, c["mode"], G.cuda() if c["mode"] == "weighted" else None,
                                        ei, eo, elig)
    if c["kind"] == "npa":
        return ops.topk_pooled_scores(c["user"][0].cuda(), c["user"][1].cuda(), c["shared"][0].cuda(), k, ei, eo, elig)
    proj, w2, b2 = c["shared"]
    return ops.topk_relu_scores(c["user"][0].cuda(), proj.cuda(), w2.cuda(), b2.cuda(), k, ei, eo, elig)


def _run(c, targets, excl=None, eligible=None, slices=0, tgt_off=None, excl_off=None):
    ti, to = C.ragged(targets)
    ei = eo = None
    if excl is not None:
        ei, eo = C.ragged(excl)
        ei, eo = ei.cuda(), (excl_off if excl_off is not None else eo).cuda()
    rank, score, ranked, status = _call(c, ti.cuda(), (tgt_off if tgt_off is not None else to).cuda(), ei, eo,
                                        eligible.cuda() if eligible is not None else None, slices)
    return rank.cpu(), score.cpu(), ranked.cpu(), int(status)


def _lists(seed, B, V):
    """Targets (0 to 4 a user, a duplicate now and then), exclusion lists (0 to 9, duplicates allowed) and a mixed mask."""
    g = torch.Generator().manual_seed(seed)
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 5, (B,), generator=g)]
    targets[0] = targets[0] or [0]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 10, (B,), generator=g)]
    eligible = (torch.rand(V, generator=g) > 0.15).to(torch.uint8)
    return targets, excl, eligible


# MINER (B, K, V, D): one user and row; Ut = 21 crossed (B = 23); K = 64: Ut = 1; K = 1: one tile of 64 users crossed
_MINER_SHAPES = [(1, 1, 1, 4), (5, 3, 130, 20), (23, 3, 129, 8), (3, 64, 300, 12), (70, 1, 700, 36)]
# DKN (B, V, Hd): Hd = 1, Hd odd and no multiple of 4, 64 users crossed, Hd = 64 (the widest proj tile)
_DKN_SHAPES = [(1, 1, 1), (65, 129, 5), (70, 700, 16), (6, 300, 64)]
# NPA (B, V, L, F): one token; two table tiles; 64 users crossed with an odd token count; F no multiple of the k-tile of 16
_NPA_SHAPES = [(1, 1, 1, 4), (3, 130, 2, 8), (65, 129, 3, 12), (70, 300, 5, 36)]
_EXACT = [("miner", s, m) for s in _MINER_SHAPES for m in ("max", "mean")] + [("dkn", s, None) for s in _DKN_SHAPES] + \
    [("npa", s, None) for s in _NPA_SHAPES]
_FAMILIES = [("miner", "max"), ("miner", "mean"), ("dkn", None), ("npa", None)]
# the shapes of the cases that are not about shapes: B users and V rows of (kind)
_SHAPE = {"miner": lambda B, V: (B, 3, V, 12), "dkn": lambda B, V: (B, V, 7), "npa": lambda B, V: (B, V, 4, 12)}
_ALL_MODES = [("miner", "max"), ("miner", "mean"), ("miner", "weighted"), ("dkn", None)]


# ---- 1. exact, with ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,mode", _EXACT)
def test_exact_with_ties(kind, shape, mode):
    c = _int_case(kind, sum(shape) * 7 + len(shape), shape, mode)
    B, V = _sizes(c)
    targets, excl, eligible = _lists(sum(shape) + 1, B, V)
    s = _scores64(c)
    rank, score, ranked, status = _run(c, targets)
    assert status == 0 and C.same((rank, score, ranked), C.expected_ranks(s, targets))
    assert bool((ranked == V).all())
    rank, score, ranked, status = _run(c, targets, excl, eligible)
    assert status == 0 and C.same((rank, score, ranked), C.expected_ranks(s, targets, excl, eligible))


@pytest.mark.parametrize("kind,shape,mode", [e for e in _EXACT if e[1][2 if e[0] == "miner" else 1] in (300, 700)])
def test_slice_counts(kind, shape, mode):
    """700 rows are 6 table tiles, 300 are 3: every slice count up to the number of tiles gives the reference."""
    c = _int_case(kind, 77, shape, mode)
    B, V = _sizes(c)
    targets, excl, eligible = _lists(78, B, V)
    want = C.expected_ranks(_scores64(c), targets, excl, eligible)
    for slices in range(0, (V + 127) // 128 + 1):
        rank, score, ranked, status = _run(c, targets, excl, eligible, slices)
        assert status == 0 and C.same((rank, score, ranked), want), slices


def _target_case(kind, mode):
    """The target lists of ``test_gpu_catalogue_rank._target_case`` over 6 users and 300 rows."""
    V = 300
    c = _int_case(kind, 41, (6, V, 64) if kind == "dkn" else _SHAPE[kind](6, V), mode)
    g = torch.Generator().manual_seed(42)
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[[7, 200]] = 0
    excl = [[], [5, 9], [150, 150, 3], [], [], [1]]
    targets = [[], torch.randperm(V, generator=g)[:32].tolist(), [17, 150, 17, 7, -1, V, 3, 299], [4], [0, 299], [200, 1, 2]]
    return c, targets, excl, eligible


@pytest.mark.parametrize("kind,mode", _FAMILIES)
def test_target_lists(kind, mode):
    """No targets, exactly 32, the same row twice, a target on the own exclusion list, an ineligible one, -1 and V."""
    c, targets, excl, eligible = _target_case(kind, mode)
    rank, score, ranked, status = _run(c, targets, excl, eligible, slices=2)
    want = C.expected_ranks(_scores64(c), targets, excl, eligible)
    assert status == E_TARGET_ROW and C.same((rank, score, ranked), want)
    r2 = rank[32:40].tolist()                                    # user 2: [17, 150, 17, 7, -1, V, 3, 299]
    assert r2[0] == r2[2] > 0 and r2[1] == r2[3] == r2[4] == r2[5] == r2[6] == 0 and r2[7] > 0
    assert bool((score[32:40][torch.tensor(r2) == 0] == NEG_INF).all())
    assert rank[-3:].tolist()[:2] == [0, 0] and int(rank[-1]) > 0 # user 5: ineligible, excluded, fine
    # no targets at all still counts the populations
    rank, score, ranked, status = _run(c, [[] for _ in range(6)], excl, eligible)
    assert status == 0 and rank.numel() == 0 and score.numel() == 0 and ranked.tolist() == [298, 296, 296, 298, 298, 297]


# ---- 2. one interest is catalogue_ranks ------------------------------------------------------------------------------------------------
def test_one_interest_returns_the_bits_of_catalogue_ranks():
    from newsreclib_amd import ops
    B, V, D = 70, 700, 36
    c = _real_case("miner", 5, (B, 1, V, D))
    targets, excl, eligible = _lists(6, B, V)
    (ti, to), (ei, eo) = C.ragged(targets), C.ragged(excl)
    ti, to, ei, eo, elig = ti.cuda(), to.cuda(), ei.cuda(), eo.cuda(), eligible.cuda()
    want = ops.catalogue_ranks(c["user"][0][:, 0].cuda(), c["shared"][0].cuda(), ti, to, ei, eo, elig)
    assert int(want[3]) == 0 and bool((want[0] > 0).any())
    for mode in R.MODES:
        out = _call(dict(c, mode=mode), ti, to, ei, eo, elig)
        assert int(out[3]) == 0 and C.same(out[:3], want[:3]), mode


# ---- 3. consistency with the top-k lists on real values -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", _ALL_MODES + [("npa", None)])
def test_consistency_with_topk_on_real_values(kind, mode):
    """rank <= 128 exactly when the target is slot rank - 1 of the family's top-k list, with the list's score bits."""
    B, V, k = 23, 1000, 128
    c = _real_case(kind, 36, {"miner": (B, 3, V, 20), "dkn": (B, V, 16), "npa": (B, V, 4, 20)}[kind], mode)
    g = torch.Generator().manual_seed(37)
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 30, (B,), generator=g)]
    extra = torch.randint(0, V, (B, 3), generator=g)
    ei, eo = C.ragged(excl)
    idx, top_score, st = _topk(c, k, ei.cuda(), eo.cuda())
    idx, top_score = idx.cpu(), top_score.cpu()
    assert int(st) == 0
    targets = [extra[b].tolist() + [int(idx[b, 0]), int(idx[b, 63]), int(idx[b, 127])] for b in range(B)]
    rank, score, ranked, status = _run(c, targets, excl)
    assert status == 0 and ranked.tolist() == [V - len(set(x)) for x in excl]
    rank2, score2 = rank.reshape(B, 6), score.reshape(B, 6)
    assert rank2[:, 3:].tolist() == [[1, 64, 128]] * B
    for b in range(B):
        for j, t in enumerate(targets[b]):
            r = int(rank2[b, j])
            assert (1 <= r <= k) == bool((idx[b] == t).any()), (b, t, r)
            assert (r == 0) == (t in excl[b])
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == t
                assert torch.equal(score2[b, j].view(torch.int32), top_score[b, r - 1].view(torch.int32))


# ---- 4. real values against float64 ----------------------------------------------------------------------------------------------------
def _check_intervals(out, s, bound, targets, excl):
    rank, score, ranked, status = out
    assert status == 0
    pop = C.population(s, excl)[0]
    intervals = C.rank_intervals(s, bound, pop, targets)
    flat = [(b, t) for b, tl in enumerate(targets) for t in tl]
    assert len(intervals) == rank.numel() == len(flat)
    for j, (iv, (b, t)) in enumerate(zip(intervals, flat)):
        if iv is None:
            assert int(rank[j]) == 0 and float(score[j]) == NEG_INF
            continue
        err = abs(float(score[j]) - float(s[b, t]))
        print(f"target {j}: rank {int(rank[j])} in [{iv[0]}, {iv[1]}]; |score - float64| = {err:.3e}, bound {float(bound[b, t]):.3e}")
        assert iv[0] <= int(rank[j]) <= iv[1] and err <= float(bound[b, t])
    assert torch.equal(ranked, pop.sum(1).to(torch.int32))


@pytest.mark.parametrize("mode", R.MODES)
def test_real_values_against_float64_interests(mode):
    d = R.real_miner()
    s, bound = R.interest_scores64(d["E"], d["T"], mode, d["G"])
    _check_intervals(_run(_miner(d["E"], d["G"], d["T"], mode), d["targets"], d["excl"]), s, bound, d["targets"], d["excl"])


def test_real_values_against_float64_pooled():
    d = R.real_npa()
    _check_intervals(_run(_npa(d["q"], d["user"], d["feat"]), d["targets"], d["excl"]), d["s"], d["bound"], d["targets"], d["excl"])


def test_real_values_against_float64_dnn():
    d = R.real_dkn()
    _check_intervals(_run(_dkn(d["q"], d["proj"], d["w2"], d["b2"]), d["targets"], d["excl"]), d["s"], d["bound"], d["targets"],
                     d["excl"])


# ---- 5. status and blanking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", _FAMILIES)
def test_status_bad_exclusion_index_is_ignored(kind, mode):
    c, targets, excl, eligible = _target_case(kind, mode)
    targets = [[t for t in tl if 0 <= t < 300] for tl in targets]
    bad = [list(x) for x in excl]
    bad[1] = [-1] + bad[1]
    bad[3] = bad[3] + [300]
    rank, score, ranked, status = _run(c, targets, bad, eligible)
    assert status == E_EXCLUDE and C.same((rank, score, ranked), C.expected_ranks(_scores64(c), targets, excl, eligible))


@pytest.mark.parametrize("kind,mode", _FAMILIES)
def test_status_bad_offsets_blank_that_user_alone(kind, mode):
    B, V = 4, 40
    c = _int_case(kind, 19, _SHAPE[kind](B, V), mode)
    s = _scores64(c)
    # exclusion offsets: user 1 runs backwards
    excl_flat, targets = list(range(12)), [[20, 1], [30], [31, 4], [32]]
    rank, score, ranked, status = _run(c, targets, [excl_flat], excl_off=torch.tensor([0, 5, 3, 8, 12]))
    assert status == E_OFFSETS
    want = C.expected_ranks(s, targets, [excl_flat[0:5], [], excl_flat[3:8], excl_flat[8:12]])
    keep = torch.tensor([True, True, False, True, True, True])
    assert torch.equal(rank[keep], want[0][keep]) and torch.equal(score[keep], want[1][keep])
    assert int(rank[2]) == 0 and float(score[2]) == NEG_INF and int(ranked[1]) == 0
    assert torch.equal(ranked[[0, 2, 3]], want[2][[0, 2, 3]])
    # target offsets: user 2 runs backwards; user 3 is empty
    flat = [3, 9, 9, 0, 21, 39, 5, 6, 7]
    rank, score, ranked, status = _run(c, [flat], tgt_off=torch.tensor([0, 4, 9, 7, 7]))
    assert status == E_TARGETS and C.same((rank, score, ranked), C.expected_ranks(s, [flat[0:4], flat[4:9], [], []]))


@pytest.mark.parametrize("kind,mode", _FAMILIES)
def test_more_than_32_targets_blank_that_user_alone(kind, mode):
    c, targets, excl, eligible = _target_case(kind, mode)
    clean = [[t for t in tl if 0 <= t < 300] for tl in targets]
    want = C.expected_ranks(_scores64(c), clean, excl, eligible)
    over = [list(tl) for tl in clean]
    over[3] = list(range(33))
    rank, score, ranked, status = _run(c, over, excl, eligible)
    assert status == E_TARGETS and torch.equal(ranked, want[2])
    n_before = sum(len(tl) for tl in over[:3])
    assert bool((rank[n_before:n_before + 33] == 0).all()) and bool((score[n_before:n_before + 33] == NEG_INF).all())
    keep = torch.ones(rank.numel(), dtype=torch.bool)
    keep[n_before:n_before + 33] = False
    drop = torch.ones(want[0].numel(), dtype=torch.bool)
    drop[n_before:n_before + 1] = False                          # (user 3 had one target in the clean case)
    assert torch.equal(rank[keep], want[0][drop]) and torch.equal(score[keep], want[1][drop])


@pytest.mark.parametrize("kind,mode", _FAMILIES)
def test_nan_table_row_is_left_out_and_flagged(kind, mode):
    B, V, nan_row = 5, 300, 140
    c = _int_case(kind, 23, _SHAPE[kind](B, V), mode)
    targets = [[nan_row, 3], [5], [141, 139], [], [nan_row]]
    table = c["shared"][0].clone()
    table[nan_row].view(-1)[-1] = float("nan")                   # (NPA: a column where q is 0 -- 0 * NaN is still NaN)
    cn = _with(c, shared=(table,) + tuple(c["shared"][1:]))
    rank, score, ranked, status = _run(cn, targets, slices=2)
    assert status == E_NAN
    elig = torch.ones(V, dtype=torch.uint8)
    elig[nan_row] = 0
    assert C.same((rank, score, ranked), C.expected_ranks(_scores64(c), targets, eligible=elig))      # as if the row were not there
    assert int(rank[0]) == 0 and int(rank[-1]) == 0 and bool((ranked == V - 1).all())
    assert _run(cn, targets, eligible=elig)[3] == 0              # a NaN row nobody may be recommended is not reported


@pytest.mark.parametrize("kind,mode,where", [("miner", "weighted", 1), ("miner", "weighted", 0), ("miner", "max", 0),
                                             ("miner", "mean", 0), ("dkn", None, 0), ("npa", None, 0), ("npa", None, 1)])
def test_nan_in_one_users_row_blanks_that_user_alone(kind, mode, where):
    """``where``: which of the user-side tensors (interests / gate, q, q / user vector) gets the NaN."""
    B, V, u = 5, 300, 2
    c = _real_case(kind, 29, _SHAPE[kind](B, V), mode)
    targets, excl, _ = _lists(30, B, V)
    targets[u] = [1, 2]
    clean = _run(c, targets, excl)
    assert clean[3] == 0
    user = [t.clone() for t in c["user"]]
    user[where][u].view(-1)[4] = float("nan")
    rank, score, ranked, status = _run(_with(c, user=tuple(user)), targets, excl)
    assert status == E_NAN and int(ranked[u]) == 0
    at = sum(len(tl) for tl in targets[:u])
    assert rank[at:at + 2].tolist() == [0, 0] and bool((score[at:at + 2] == NEG_INF).all())
    keep = torch.ones(rank.numel(), dtype=torch.bool)
    keep[at:at + 2] = False
    others = torch.arange(B) != u
    assert torch.equal(rank[keep], clean[0][keep]) and torch.equal(score[keep].view(torch.int32), clean[1][keep].view(torch.int32))
    assert torch.equal(ranked[others], clean[2][others])


# ---- 6. invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", _ALL_MODES + [("npa", None)])
def test_invariance(kind, mode, engine):
    """Bit-equal ranks, scores and populations for the whole batch against each user alone and against the users in reverse order,
    across slice counts and across the two GEMM engine settings (the f32 result is recorded in the first parametrisation and
    compared in the second)."""
    from newsreclib_amd import _lib
    B, V = 23, 700
    c = _real_case(kind, 31, {"miner": (B, 3, V, 20), "dkn": (B, V, 16), "npa": (B, V, 4, 20)}[kind], mode)
    g = torch.Generator().manual_seed(32)
    targets = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 5, (B,), generator=g)]
    excl = [torch.randint(0, V, (int(n),), generator=g).tolist() for n in torch.randint(0, 30, (B,), generator=g)]

    def run(case, tl, el, slices=0):
        out = _run(case, tl, el, slices=slices)
        assert out[3] == 0
        return out[0], C.bits(out[1]), out[2]

    base = run(c, targets, excl)
    for slices in (1, 2, 5):
        assert C.same(run(c, targets, excl, slices), base), slices
    singles = [run(_take(c, slice(b, b + 1)), [targets[b]], [excl[b]]) for b in range(B)]
    assert C.same(tuple(torch.cat([s[i] for s in singles]) for i in range(3)), base)
    rev = run(_take(c, torch.arange(B - 1, -1, -1)), targets[::-1], excl[::-1])
    per_user = torch.split(base[0], [len(t) for t in targets]), torch.split(base[1], [len(t) for t in targets])
    assert torch.equal(rev[0], torch.cat(per_user[0][::-1])) and torch.equal(rev[1], torch.cat(per_user[1][::-1]))
    assert torch.equal(rev[2], base[2].flip(0))
    key = ("invariance", kind, mode)
    if engine == "f32":
        _F32[key] = base
    else:
        if key not in _F32:                                      # (this parametrisation selected alone)
            _lib.set_gemm_engine("f32")
            _F32[key] = run(c, targets, excl)
            _lib.set_gemm_engine(engine)
        assert C.same(base, _F32[key])


# ---- 7. no read-back, memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("miner", "weighted"), ("dkn", None), ("npa", None)])
def test_rank_entries_do_not_synchronise_with_the_host(kind, mode):
    c = _int_case(kind, 3, _SHAPE[kind](5, 200), mode)
    c = dict(c, user=tuple(t.cuda() for t in c["user"]), shared=tuple(t.cuda() for t in c["shared"]))
    (ti, to), (ei, eo) = C.ragged([[1, 2], [], [5], [7, 7], [199]]), C.ragged([[1], [], [5, 6], [], []])
    ti, to, ei, eo, elig = ti.cuda(), to.cuda(), ei.cuda(), eo.cuda(), torch.ones(200, dtype=torch.uint8).cuda()
    _call(c, ti, to, ei, eo, elig)                               # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not C.sync_debug_honoured():
            pytest.skip("this torch build does not raise on synchronising calls under set_sync_debug_mode('error')")
        rank, score, ranked, status = _call(c, ti, to, ei, eo, elig)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status) == 0 and rank.shape == (6,) and ranked.shape == (5,)


@pytest.mark.parametrize("kind,mode", [("miner", "weighted"), ("dkn", None), ("npa", None)])
def test_peak_memory_is_far_below_the_score_matrix(kind, mode):
    """(NPA: far below (B, V) as well, so nothing of the size of the targets' feature maps, let alone (B, V, L), is written.)"""
    B, V = 256, 60000
    c = _real_case(kind, 2, {"miner": (B, 3, V, 64), "dkn": (B, V, 16), "npa": (B, V, 2, 16)}[kind], mode)
    c = dict(c, user=tuple(t.cuda() for t in c["user"]), shared=tuple(t.cuda() for t in c["shared"]))
    g = torch.Generator().manual_seed(2)
    ti = torch.randint(0, V, (B * 3,), generator=g).cuda()
    to = (torch.arange(B + 1) * 3).cuda()
    small = dict(c, user=tuple(t[:2] for t in c["user"]), shared=(c["shared"][0][:256],) + tuple(c["shared"][1:]))
    _call(small, ti[:6] % 256, to[:3])                           # library loaded, kernels resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    out = _call(c, ti, to)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - live
    print(f"peak above the inputs: {peak} bytes; score matrix: {B * V * 4} bytes")
    assert peak < B * V * 4 / 8
    assert int(out[3]) == 0 and bool((out[0] >= 1).all()) and bool((out[2] == V).all())


# ---- 8. wiring ----------------------------------------------------------------------------------------------------------------------------
def _check_against_recommend(recommend, rank_clicks, lists, hist, hs, V, k=128, **kw):
    """``rank_clicks`` over clicks drawn from the top list, at random and from the history against ``recommend`` at k."""
    B = int(hs.numel())
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0                                              # the padding row
    idx, top_score, st = recommend(hist.cuda(), hs, k, eligible=eligible, **kw)
    idx, top_score = idx.cpu(), top_score.cpu()
    assert int(st) == 0
    g = torch.Generator().manual_seed(6)
    clicks = [[int(idx[b, 0]), int(idx[b, 3])] + torch.randint(0, V, (b % 4,), generator=g).tolist() + [int(lists[b][0])]
              for b in range(B)]
    click_idx, cs = torch.tensor([c for cl in clicks for c in cl]), torch.tensor([len(cl) for cl in clicks])
    rank, score, ranked, status = rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, eligible=eligible, **kw)
    assert int(status) == 0 and rank.shape == (int(cs.sum()),) and ranked.shape == (B,)
    rank, score, ranked = rank.cpu(), score.cpu(), ranked.cpu()
    assert ranked.tolist() == [V - len(set(lists[b].tolist()) | {0}) for b in range(B)]    # all but the padding row and the history
    at = 0
    for b in range(B):
        assert int(rank[at]) == 1 and int(rank[at + 1]) == 4
        for c in clicks[b]:
            r = int(rank[at])
            assert (1 <= r <= k) == bool((idx[b] == c).any()), (b, c, r)
            if 1 <= r <= k:
                assert int(idx[b, r - 1]) == c
                assert torch.equal(score[at].view(torch.int32), top_score[b, r - 1].view(torch.int32))
            if c in lists[b].tolist() or c == 0:
                assert r == 0 and float(score[at]) == NEG_INF
            at += 1
    # without the exclusion a click from the history ranks like any other row
    rank2, _, ranked2, _ = rank_clicks(hist.cuda(), hs, click_idx.cuda(), cs, exclude_history=False, **kw)
    assert bool((ranked2 == V).all()) and bool((rank2 >= 1).all())


def _check_evaluate_full_rank(cache, rank_clicks, lists, hs, V, parts, uidx=None):
    """Two batches give ``full_rank_metrics`` of the two ``rank_clicks_*`` calls (a batch's longest history enters the user side of
    some modules, so the split is part of the input); a status flag is passed on as ONE warning."""
    import warnings

    from newsreclib_amd.evaluation import evaluate_full_rank
    from newsreclib_amd.metrics import full_rank_metrics
    B = int(hs.numel())
    g = torch.Generator().manual_seed(13)
    clicks = [torch.randint(1, V, (int(n),), generator=g) for n in torch.randint(0, 5, (B,), generator=g)]
    clicks[0] = torch.tensor([1, 2])
    users = [{"hist": lists[b], "clicks": clicks[b]} for b in range(B)]
    if uidx is not None:
        users = [dict(u, user_idx=uidx[b]) for b, u in enumerate(users)]
    eligible = torch.ones(V, dtype=torch.uint8)
    eligible[0] = 0
    outs = []
    for lo, hi in parts:
        h, c = torch.cat([lists[b] for b in range(lo, hi)]), torch.cat([clicks[b] for b in range(lo, hi)])
        outs.append(rank_clicks(h.cuda(), hs[lo:hi], c.cuda(), torch.tensor([len(clicks[b]) for b in range(lo, hi)]),
                                eligible=eligible, **({"user_idx": uidx[lo:hi]} if uidx is not None else {})))
    assert all(int(o[3]) == 0 for o in outs)
    want = full_rank_metrics(torch.cat([o[0] for o in outs]).cpu(), torch.tensor([len(c) for c in clicks]),
                             torch.cat([o[2] for o in outs]).cpu(), (5, 10))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # no flag, no warning
        got = evaluate_full_rank(cache, users, (5, 10), batch_size=parts[0][1], eligible=eligible)
    assert got == want and set(got) == {"mrr", "auc_user", "ndcg@5", "ndcg@10", "recall@5", "recall@10", "hit@5", "hit@10"}
    users[1] = dict(users[1], clicks=torch.tensor([V]))          # outside the table: flag 32 in the first batch only
    with pytest.warns(UserWarning, match=r"evaluate_full_rank: a target index is outside \[0, V\)") as rec:
        evaluate_full_rank(cache, users, (5, 10), batch_size=parts[0][1], eligible=eligible)
    assert len(rec) == 1


@pytest.mark.parametrize("score_type", R.MODES)
def test_rank_clicks_interests_against_recommend_interests(score_type, tmp_path):
    mod, cfg, cache, hist, hs = builders.miner_cache("miner_tiny_no_bias", score_type, tmp_path)
    mod.train()
    assert mod.interest_score_mode == score_type
    V, B = cache.table.num_news, int(hs.numel())
    lists = list(torch.split(hist, hs.tolist()))
    _check_against_recommend(cache.recommend_interests, cache.rank_clicks_interests, lists, hist, hs, V)
    assert mod.training                                          # the mode is restored
    _check_evaluate_full_rank(cache, cache.rank_clicks_interests, lists, hs, V, [(0, B - 1), (B - 1, B)] if B > 1 else [(0, B)])
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        cache.rank_clicks(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="no `dnn_predictor_scorer`"):
        cache.rank_clicks_dnn(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))


@pytest.mark.parametrize("late_fusion", [False, True])
def test_rank_clicks_dnn_against_recommend_dnn(late_fusion):
    from newsreclib_amd.evaluation import DeviceNewsTable, NewsVectorCache
    mod, attrs = builders.tiny_dkn(late_fusion=late_fusion)
    mod.train()
    cache = NewsVectorCache(mod, DeviceNewsTable(attrs), chunk=32)
    V, B = 50, 6
    lists, hist, hs = builders.hist_batch(V)[:3]
    _check_against_recommend(cache.recommend_dnn, cache.rank_clicks_dnn, lists, hist, hs, V)
    assert mod.training and (cache.projection is None) == late_fusion
    _check_evaluate_full_rank(cache, cache.rank_clicks_dnn, lists, hs, V, [(0, 4), (4, 6)])
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        cache.rank_clicks(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="no `multi_interest_scorer`"):
        cache.rank_clicks_interests(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))


@pytest.mark.parametrize("late_fusion", [False, True])
def test_rank_clicks_pooled_against_recommend_pooled(late_fusion):
    mod, table = builders.tiny_npa(late_fusion)
    mod.train()
    cache = mod.feature_cache(table, chunk=32)
    V, B = 50, 6
    lists, hist, hs = builders.hist_batch(V)[:3]
    uidx = torch.tensor([3, 1, 4, 1, 5, 8])
    _check_against_recommend(cache.recommend_pooled, cache.rank_clicks_pooled, lists, hist, hs, V, user_idx=uidx)
    assert mod.training                                          # the mode is restored
    _check_evaluate_full_rank(cache, cache.rank_clicks_pooled, lists, hs, V, [(0, 4), (4, 6)], uidx)
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        cache.rank_clicks(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))
    with pytest.raises(ValueError, match="needs user_idx"):
        cache.rank_clicks_pooled(hist.cuda(), hs, torch.ones(B, dtype=torch.int64).cuda(), torch.ones(B, dtype=torch.int64))
    mod.eval()


def test_the_other_caches_still_refuse():
    from newsreclib_amd import evaluation as E
    from newsreclib_amd.npa_module import NPAModule
    args = (torch.ones(6, dtype=torch.int64).cuda(), torch.ones(6, dtype=torch.int64), torch.ones(6, dtype=torch.int64).cuda(),
            torch.ones(6, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        E.NpaFeatureCache(object.__new__(NPAModule), None).rank_clicks(*args)
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        object.__new__(E.MannerVectorCache).rank_clicks(*args)
    cache = object.__new__(E.MannerVectorCache)
    cache.module, cache.table = object(), type("T", (), {"device": "cuda"})()
    with pytest.raises(NotImplementedError, match="only the dot-product families are served"):
        E.evaluate_full_rank(cache, [{"hist": torch.tensor([1]), "clicks": torch.tensor([2])}])
