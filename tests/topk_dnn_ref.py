"""Shared by test_topk_dnn_host.py and test_gpu_topk_dnn.py: the inputs of the real-value case, the float64 value of DKN's
factored click score and its derived fp32 error bound.  Population, order and the floor check are ``tests/catalogue_ref.py``'s.

The factored score: with ``pred_w1 = [Wc | Wu]``, ``P = T Wc^T`` (V, Hd) and ``q = U Wu^T + b1`` (B, Hd),

    score(u, v) = b2 + sum_j w2[j] relu(P[v, j] + q[u, j]).

Bound (derived, not measured), EPS = 2^-23, for fp32 evaluation of P and q as length-``dim`` dot products in any order, one
rounded addition, and the fma chain over j:

    e_P   = dim EPS (|T| |Wc|^T)                     an fp32 dot product of length dim
    e_q   = (dim + 1) EPS (|U| |Wu|^T + |b1|)        the same, and the bias addition
    bound = sum_j |w2_j| (e_P + e_q + EPS (|P_j| + |q_j|)) + (Hd + 1) EPS (sum_j |w2_j| h_j + |b2|)

relu is 1-Lipschitz, so the error of x = P + q (its operands' errors and the addition's rounding) passes to h unamplified; the
last term is the Hd roundings of the chain.  ``U`` is taken as given (fp32): the user vector is compared bit for bit with the
click kernel's elsewhere."""
import functools

import torch

EPS = 2.0 ** -23
REAL = dict(B=37, V=5000, dim=400, Hd=16, k=10, seed=5)


def make_weights(g, dim, Hd):
    """(att, pred): (w1, b1, w2, b2) each; W1 scaled by 1 / sqrt(2 dim), w2 by 1 / sqrt(Hd), biases 0.1 N(0, 1)."""
    def dnn():
        return [torch.randn(Hd, 2 * dim, generator=g) / (2 * dim) ** 0.5, 0.1 * torch.randn(Hd, generator=g),
                torch.randn(1, Hd, generator=g) / Hd ** 0.5, 0.1 * torch.randn(1, generator=g)]
    return dnn(), dnn()


@functools.lru_cache(maxsize=None)
def real_case():
    """hist rows (n_hist, dim) N(0, 1) with ragged sizes (an empty history and several of one row among them), the table
    (V, dim) N(0, 1), the weights, and exclusion lists of 0 - 50 rows.  Treated as read-only by every test."""
    c = REAL
    g = torch.Generator().manual_seed(c["seed"])
    sizes = torch.randint(1, 31, (c["B"],), generator=g)
    sizes[3], sizes[4], sizes[5], sizes[6] = 0, 1, 1, 1
    hist = torch.randn(int(sizes.sum()), c["dim"], generator=g)
    table = torch.randn(c["V"], c["dim"], generator=g)
    att, pred = make_weights(g, c["dim"], c["Hd"])
    excl = [torch.randint(0, c["V"], (int(n),), generator=g).tolist() for n in torch.randint(0, 51, (c["B"],), generator=g)]
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    return dict(hist=hist, sizes=sizes, off=off, table=table, att=att, pred=pred, excl=excl)


def user_vectors(hist, off, att, dtype=torch.float32):
    """The DKN user vector on the CPU: softmax over s_i = v . h_i with v = W1[:, dim:]^T w2 (the attention DNN is affine: the
    candidate's share cancels), zero for an empty history."""
    dim = hist.shape[1]
    w1, w2 = att[0].to(dtype), att[2].to(dtype)
    v = (w2.reshape(1, -1) @ w1[:, dim:]).reshape(-1)
    out = torch.zeros(off.numel() - 1, dim, dtype=dtype)
    for b in range(off.numel() - 1):
        h = hist[int(off[b]):int(off[b + 1])].to(dtype)
        if h.shape[0]:
            out[b] = torch.softmax(h @ v, 0) @ h
    return out


def scores64(U, T, pred):
    """float64 score (B, V) of the factored predictor from fp32 ``U`` (B, dim) and ``T`` (V, dim), and its fp32 bound (B, V)."""
    dim = T.shape[1]
    w1, b1, w2, b2 = [t.double() for t in pred]
    Hd = w1.shape[0]
    wc, wu, w2 = w1[:, :dim], w1[:, dim:], w2.reshape(-1)
    U, T = U.double(), T.double()
    P, q = T @ wc.T, U @ wu.T + b1
    e_p = dim * EPS * (T.abs() @ wc.abs().T)
    e_q = (dim + 1) * EPS * (U.abs() @ wu.abs().T + b1.abs())
    aw = w2.abs()
    score = torch.empty(U.shape[0], T.shape[0], dtype=torch.float64)
    bound = torch.empty_like(score)
    for b in range(U.shape[0]):                             # (V, Hd) at a time
        h = torch.relu(P + q[b])
        score[b] = h @ w2 + b2
        bound[b] = (e_p + e_q[b] + EPS * (P.abs() + q[b].abs())) @ aw + (Hd + 1) * EPS * (h @ aw + b2.abs())
    return score, bound


def emulate_fp32(U, T, pred):
    """The factored score in fp32 on the CPU: P and q by fp32 matmul, one addition, x < 0 ? 0 : x, the chain in ascending j
    (multiplication and addition rounded separately: two roundings of 2^-24 per step, inside the chain's (Hd + 1) EPS term)."""
    dim = T.shape[1]
    w1, b1, w2, b2 = pred
    P, q = T @ w1[:, :dim].T, U @ w1[:, dim:].T + b1
    w2 = w2.reshape(-1)
    out = torch.empty(U.shape[0], T.shape[0], dtype=torch.float32)
    for b in range(U.shape[0]):
        x = P + q[b]
        h = torch.where(x < 0, torch.zeros_like(x), x)
        s = b2.reshape(()).expand(T.shape[0]).clone()
        for j in range(w2.numel()):
            s = s + w2[j] * h[:, j]
        out[b] = s
    return out


def relu_scores64(q, proj, w2, b2):
    """(B, V) float64 scores from q (B, Hd), proj (V, Hd): exact for the small-integer cases."""
    h = torch.relu(proj.double()[None, :, :] + q.double()[:, None, :])
    return h @ w2.double().reshape(-1) + b2.double().reshape(())
