"""The relation head (egtr_amd/csrc/rel_head.hip, rel_head_bf16.hip) restated in plain torch, float64 by default, and the
deterministic "grid" inputs on which every kernel variant has to return the same bits.  No GPU, no product import.

Tensors (the layout of the C entries): gate_q / gate_k [B, N, T], uq / uk [B, N, T, 512] (channels 0-255 the relation MLP, 256-511
the connectivity MLP), b1 [512], w2* [256, 256], b2* [256], w3r [R, 256], b3r [R], w3c [1, 256], b3c [1], triplet [C1, C1, R],
node_cls [B, N] int64.  The saved activations are [2 (mlp), B N N, 256], post-ReLU.

The grid (``grid_inputs`` / ``grid_dh1``): gate logits in {-200, 0, 200}, tables even integers in [-6, 6], biases integers in
[-4, 4], two (W2) / three (W3) entries of +-1 per weight row, frequency bias integers in [-8, 8], dh1 integers in [-2, 2].  Every
gate is exactly 0, 0.5 or 1 (fp32: exp(200) = inf, exp(-200) = 0, exp(0) = 1), every intermediate an integer or half-integer far
below 256: exact in bf16, every fp32 sum exact in any order.  tests/test_relation_head_cases_cpu.py asserts all of that per case."""
import torch

HD = 256
NAMES = ("gate_q", "gate_k", "uq", "uk", "b1", "w2r", "b2r", "w3r", "b3r", "w2c", "b2c", "w3c", "b3c")


# ---------------------------------------------------------------------------------------------------------------- forward
def gates(gate_q, gate_k):
    """g[b, i, j, t] = 1 / (1 + exp(-(gate_q[b, i, t] + gate_k[b, j, t]))), the form the kernels evaluate"""
    return 1.0 / (1.0 + torch.exp(-(gate_q[:, :, None, :] + gate_k[:, None, :, :])))


def forward(d, dtype=torch.float64, round_bf16=False, drop_slot=None, swap_uk=False, skip_last_col=False, swap_bias=False):
    """d: dict of the NAMES (+ optional "triplet", "node_cls").  Returns (rel [B, N, N, R], conn [B, N, N], gate_mean [T],
    h1 [2, B N N, 256], h2 [2, B N N, 256]) in ``dtype``.  ``round_bf16``: h1 and h2 pass through bfloat16 before the next layer
    (what the bf16 kernels do to their operands).  The remaining switches build deliberately WRONG compositions (teeth of the
    bitwise assertions): ``drop_slot`` t leaves slot t out of the gated sum, ``swap_uk`` looks uk up by the subject, ``swap_bias``
    indexes the frequency bias [cls_j, cls_i], ``skip_last_col`` leaves object column N - 1 unwritten (NaN) in every output."""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    B, N, T = t["gate_q"].shape
    P = B * N * N
    g = gates(t["gate_q"], t["gate_k"])
    gs = g.clone()
    if drop_slot is not None:
        gs[..., drop_slot] = 0
    pre = torch.einsum("bijt,bitc->bijc", gs, t["uq"]) + t["b1"]
    pre = pre + (torch.einsum("bijt,bitc->bijc", gs, t["uk"]) if swap_uk else torch.einsum("bijt,bjtc->bijc", gs, t["uk"]))
    h1 = torch.relu(pre)

    def rb(x):
        return x.bfloat16().to(dtype) if round_bf16 else x

    F = torch.nn.functional
    h2r = torch.relu(F.linear(rb(h1[..., :HD]), t["w2r"], t["b2r"]))
    h2c = torch.relu(F.linear(rb(h1[..., HD:]), t["w2c"], t["b2c"]))
    rel = F.linear(rb(h2r), t["w3r"], t["b3r"])
    conn = F.linear(rb(h2c), t["w3c"].reshape(1, HD), t["b3c"].reshape(1))[..., 0]
    if d.get("triplet") is not None:
        tr, nc = t["triplet"], t["node_cls"]
        bias = torch.stack([tr[nc[b]][:, nc[b]] for b in range(B)], 0)      # [b, i, j, :] = triplet[cls_i, cls_j]
        rel = rel + (bias.transpose(1, 2) if swap_bias else bias)
    gm = g.reshape(-1, T).mean(0)
    h1s = torch.stack([h1[..., :HD].reshape(P, HD), h1[..., HD:].reshape(P, HD)], 0)
    h2s = torch.stack([h2r.reshape(P, HD), h2c.reshape(P, HD)], 0)
    if skip_last_col:
        nan = float("nan")
        rel[:, :, N - 1], conn[:, :, N - 1] = nan, nan
        h1s.view(2, B, N, N, HD)[:, :, :, N - 1] = nan
        h2s.view(2, B, N, N, HD)[:, :, :, N - 1] = nan
    return rel, conn, gm, h1s, h2s


def gate_mean_exact(gate_q, gate_k):
    """The mean gate per slot of GRID logits as an exact count: (#(g = 1) + 0.5 #(g = 0.5)) / (B N N), in float64"""
    z = gate_q.double()[:, :, None, :] + gate_k.double()[:, None, :, :]
    T = z.shape[-1]
    ones = (z > 0).reshape(-1, T).sum(0).double()
    halves = (z == 0).reshape(-1, T).sum(0).double()
    return (ones + 0.5 * halves) / (z.numel() // T)


# --------------------------------------------------------------------------------------------------------------- backward
def backward_pairs(dh1, gate_q, gate_k, uq, uk, dtype=torch.float64, order="einsum", skip_from=None, omit_uk=False,
                   want_mag=True):
    """The pairwise part of the backward from its formulas (the comment above rel_head_bwd_pairs_f32), no autograd:
        duq[i,t,:] = sum_j g[i,j,t] dh1[i,j,:]        duk[j,t,:] = sum_i g[i,j,t] dh1[i,j,:]
        dg[i,j,t]  = dh1[i,j,:] . (uq[i,t,:] + uk[j,t,:])        dz = dg g (1 - g)
        dgate_q[i,t] = sum_j dz[i,j,t]                dgate_k[j,t] = sum_i dz[i,j,t]
    dh1: [2, B N N, 256] (gradient of the pre-ReLU layer-1 value, both MLPs).  Returns (out, mag), two dicts with the keys
    duq, duk, dgate_q, dgate_k, dz ([B, N, N, T]): ``mag`` is the same sum over the ABSOLUTE values of the terms (of the products
    that make up dg, times g (1 - g), for dz and the gate gradients) -- the scale of a worst-case rounding bound (None without
    ``want_mag``).
    ``order``: "einsum", or "loop" = the running index m one at a time, from the top down (another fp32 summation order).
    Teeth: ``skip_from`` m leaves the terms of running index >= m out of duq / duk / dgate_*; ``omit_uk`` drops the uk half of dg."""
    B, N, T = gate_q.shape
    gq, gk, uq, uk = (x.to(dtype) for x in (gate_q, gate_k, uq, uk))
    D = torch.cat([dh1[0].reshape(B, N, N, HD), dh1[1].reshape(B, N, N, HD)], -1).to(dtype)   # [B, i, j, 512]
    g = gates(gq, gk)
    lim = N if skip_from is None else min(N, skip_from)

    def sums(Dx, uqx, ukx):
        dgq_ = torch.einsum("bijc,bitc->bijt", Dx, uqx)
        dg = dgq_ if omit_uk else dgq_ + torch.einsum("bijc,bjtc->bijt", Dx, ukx)
        dz = dg * g * (1 - g)
        if order == "einsum":
            duq = torch.einsum("bijt,bijc->bitc", g[:, :, :lim], Dx[:, :, :lim])
            duk = torch.einsum("bijt,bijc->bjtc", g[:, :lim], Dx[:, :lim])
            dgq, dgk = dz[:, :, :lim].sum(2), dz[:, :lim].sum(1)
        else:
            duq, duk = torch.zeros_like(uqx), torch.zeros_like(ukx)
            dgq, dgk = torch.zeros_like(gq), torch.zeros_like(gk)
            for m in range(lim - 1, -1, -1):
                duq += g[:, :, m, :, None] * Dx[:, :, m, None, :]
                duk += g[:, m, :, :, None] * Dx[:, m, :, None, :]
                dgq += dz[:, :, m]
                dgk += dz[:, m]
        return dict(duq=duq, duk=duk, dgate_q=dgq, dgate_k=dgk, dz=dz)

    return sums(D, uq, uk), (sums(D.abs(), uq.abs(), uk.abs()) if want_mag else None)


# ------------------------------------------------------------------------------------------------------------ grid inputs
def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _signed_rows(g, rows, per_row):
    """[rows, 256]: ``per_row`` entries of +-1 at distinct columns of every row, zero elsewhere"""
    w = torch.zeros(rows, HD)
    cols = torch.rand(rows, HD, generator=g).argsort(1)[:, :per_row]
    w.scatter_(1, cols, _ints(g, 0, 1, (rows, per_row)) * 2 - 1)
    return w


def sweep_slots(B, N, T):
    """(a [B, N - 1], c [B, N - 1]): the slot that subject i < N - 1 (a) / object j < N - 1 (c) of image b opens in the
    slot-sweep variant; a and c of one image together run through consecutive slots, the next image goes on where it ended"""
    n = N - 1
    idx = torch.arange(n)
    a = torch.stack([(idx + 2 * n * b) % T for b in range(B)]) if n else torch.zeros(B, 0, dtype=torch.long)
    c = torch.stack([(idx + 2 * n * b + n) % T for b in range(B)]) if n else torch.zeros(B, 0, dtype=torch.long)
    return a, c


def grid_inputs(seed, B, N, T, R, C1=0, sweep=False):
    """The grid inputs as a dict of float32 tensors (NAMES, + "triplet" / "node_cls" when C1 > 0; node_cls holds 0 and C1 - 1).
    ``sweep``: the slot-sweep gate variant.  Subject i < N - 1 has +200 at slot a[b, i] and -200 elsewhere, and so has object
    j < N - 1 at slot c[b, j] (``sweep_slots``); subject N - 1 and object N - 1 are all 0.  So pair (i, N - 1) has slot a[b, i] as
    its ONLY open slot (g = 1, all others 0) and pair (N - 1, j) slot c[b, j]: each slot index t, 8 and 9 of the second operand
    half included, decides alone what a pair returns.  Pairs of two opened rows have one gate of 1 (same slot) or two of 0.5."""
    g = torch.Generator().manual_seed(seed)
    d = {}
    d["gate_q"] = 200.0 * _ints(g, -1, 1, (B, N, T))
    d["gate_k"] = 200.0 * _ints(g, -1, 1, (B, N, T))
    if sweep:
        a, c = sweep_slots(B, N, T)
        for key, slot in (("gate_q", a), ("gate_k", c)):
            x = torch.full((B, N, T), -200.0)
            x[:, N - 1] = 0.0
            if N > 1:
                x[:, :N - 1].scatter_(2, slot[:, :, None], 200.0)
            d[key] = x
    d["uq"] = 2.0 * _ints(g, -3, 3, (B, N, T, 2 * HD))
    d["uk"] = 2.0 * _ints(g, -3, 3, (B, N, T, 2 * HD))
    d["b1"] = _ints(g, -4, 4, (2 * HD,))
    d["w2r"], d["b2r"] = _signed_rows(g, HD, 2), _ints(g, -4, 4, (HD,))
    d["w3r"], d["b3r"] = _signed_rows(g, R, 3), _ints(g, -4, 4, (R,))
    d["w2c"], d["b2c"] = _signed_rows(g, HD, 2), _ints(g, -4, 4, (HD,))
    d["w3c"], d["b3c"] = _signed_rows(g, 1, 3), _ints(g, -4, 4, (1,))
    if C1:
        d["triplet"] = _ints(g, -8, 8, (C1, C1, R))
        nc = torch.randint(0, C1, (B, N), generator=g)
        nc[:, 0] = 0
        nc[:, N - 1] = C1 - 1 if N > 1 else 0
        if N == 1 and B > 1:
            nc[B - 1, 0] = C1 - 1
        d["node_cls"] = nc
    return d


def grid_dh1(seed, B, N):
    """[2, B N N, 256] float32 integers in [-2, 2]"""
    g = torch.Generator().manual_seed(seed)
    return _ints(g, -2, 2, (2, B * N * N, HD))


def random_inputs(seed, B, N, T, R, C1=0):
    """Standard-normal inputs of the same shapes (weights scaled by 1 / 16 = 256 ** -0.5)"""
    g = torch.Generator().manual_seed(seed)
    shapes = dict(gate_q=(B, N, T), gate_k=(B, N, T), uq=(B, N, T, 2 * HD), uk=(B, N, T, 2 * HD), b1=(2 * HD,), w2r=(HD, HD),
                  b2r=(HD,), w3r=(R, HD), b3r=(R,), w2c=(HD, HD), b2c=(HD,), w3c=(1, HD), b3c=(1,))
    d = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    for k in ("w2r", "w3r", "w2c", "w3c"):
        d[k] = d[k] / 16
    if C1:
        d["triplet"] = torch.randn(C1, C1, R, generator=g)
        d["node_cls"] = torch.randint(0, C1, (B, N), generator=g)
    return d


# ------------------------------------------------------------------------------------------------------------ the cases
# (B, N, T, R, C1, sweep) of every grid launch of tests/test_gpu_relation_head_edges.py; the CPU file proves the exactness claim for
# each, the GPU file runs them
T_SWEEP = [(2, 9, T, 33, 0, False) for T in range(1, 11)] + [(2, 9, T, 33, 0, True) for T in (7, 9, 10)]
N_SWEEP = [(3, N, 7, 50, 12, False) for N in (1, 3, 4, 5, 8, 12, 31, 32, 33, 65)]
PERSISTENT = [(5, 65, 7, 50, 0, False)]
R_SWEEP = [(2, 9, 7, R, C1, False) for R in (1, 31, 32, 33, 60, 61, 64) for C1 in (0, 5)]
FORWARD_CASES = T_SWEEP + N_SWEEP + PERSISTENT + R_SWEEP
# (B, N, T) of the backward: every T; the four-wave split of the running index; both sides of the 256 chunk
BACKWARD_CASES = ([(2, 9, T) for T in range(1, 11)] + [(2, N, 7) for N in (1, 3, 4, 5, 63, 64, 65)]
                  + [(1, N, T) for N in (255, 256, 257) for T in (2, 10)])
BACKWARD_REAL = [(2, 40, 7), (1, 257, 4)]


def case_seed(*case):
    return 1000 + sum((i + 1) * 131 * int(v) for i, v in enumerate(case))


def case_id(case):
    return "-".join(str(int(v)) for v in case)


def backward_bound(mag, N):
    """|got - ref| <= (n + 8) 2^-24 mag per element, n the number of terms summed into it: N for duq / duk, 512 for dz, N + 512
    for the gate gradients; the 8 covers the sigmoid, the products and the four-way wave merge"""
    n = dict(duq=N, duk=N, dz=512, dgate_q=N + 512, dgate_k=N + 512)
    return {k: (n[k] + 8) * 2.0 ** -24 * mag[k] for k in mag}
