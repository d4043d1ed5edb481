"""Float64 restatement of the MSDA forward / backward with error budgets, the window bookkeeping of the value-tile kernel
restated in plain Python, and the constructed cases of tests/test_gpu_msda_windows.py.  CPU only; calls neither
oracle/msda.py nor any kernel (tests/test_msda_cases_cpu.py compares it with the oracle and with torch autograd).

Exact geometry.  Every sampling coordinate used here is a multiple of 2^-12 in [-1, 2] and every H, W is at most 512.  Then
loc * W is a multiple of 2^-12 below 1024 in magnitude (22 bits), so ``loc * W - 0.5``, its floor, lh, lw, hh, hw are exact in
fp32 with or without a fused multiply-add, and hh * hw is a multiple of 2^-24 that is at most 1: the kernels' bilinear
weights, corner indices and range decisions equal the float64 ones bit for bit.  grad_loc -- discontinuous at integer pixel
coordinates -- therefore has no ambiguous element.  ``assert_exact_geometry`` checks a case against these conditions directly.

Operand grids.  attn_weight is drawn on multiples of 2^-8 in [0, 1/8], grad_out on multiples of 2^-6 in [-4, 4]; value is a
full-mantissa normal.  attn * grad_out is then exact (16 bits) and a contribution w * attn * grad_out to grad_value is, after its
fp32 rounding, a multiple of 2^-38 -- and of 2^-36 on the levels of the two cases beyond 65 536 pixels, whose weights are
multiples of 2^-22.  The deterministic route converts with a unit of 2^-k, k = 61 - (ea + eg + en) (csrc/fixed_accum.h): with
max attn = 2^-3 < 2^-2, max|grad_out| <= 4 < 2^3 and Lq * 16 <= 2^21 terms k >= 39 (44 at S = 2720), so its conversion to fixed
point is exact and the fp32 budget below applies to that route unchanged.  (With arbitrary operands an element made of one contribution far below
2^-k could not meet an element-wise relative bound.)  The fp32 routes still round: w * (attn * grad_out) has up to 40 bits.

Budgets.  ``msda_backward_budget`` returns next to each float64 gradient the sum of the absolute values of the terms that were
added to it and, for grad_value, the number of nonzero terms per element: the tests bound the fp32 error element by element by
(number of roundings) * 2^-24 * (that sum), which holds for any order of addition.
"""
import numpy as np
import torch

GRID = 4096          # sampling coordinates are multiples of 1 / GRID
M, D = 8, 32         # heads, channels per head of the fast kernels
TQ = 8               # a query tile is TQ x TQ pixels of one level (msda_common.h: make_tile_map<8, 8>)
NPX = 32             # workgroups per head of the value-tile kernel (kBwdGrid / 8)
F64 = torch.float64


def quantize_loc(loc):
    """Nearest multiple of 2^-12 (the dtype is kept; exact for fp32 in [-1, 2])."""
    return torch.round(loc * GRID) / GRID


def level_starts(shapes):
    out, acc = [], 0
    for h, w in shapes:
        out.append(acc)
        acc += h * w
    return out


def assert_exact_geometry(shapes, loc):
    """The conditions of the module docstring, and their consequence checked directly: the fp32 evaluation of the pixel
    coordinates and of the four bilinear weights equals the float64 one."""
    assert loc.dtype == torch.float32
    assert all(1 <= h <= 512 and 1 <= w <= 512 for h, w in shapes)
    k = loc.double() * GRID
    assert bool((k == k.round()).all()) and float(loc.min()) >= -1.0 and float(loc.max()) <= 2.0
    for l, (H, W) in enumerate(shapes):
        for c, n in ((0, W), (1, H)):
            v32 = loc[:, :, :, l, :, c] * float(n) - 0.5
            v64 = loc[:, :, :, l, :, c].double() * n - 0.5
            assert v32.dtype == torch.float32 and bool((v32.double() == v64).all())
        x32, y32 = loc[:, :, :, l, :, 0] * float(W) - 0.5, loc[:, :, :, l, :, 1] * float(H) - 0.5
        lw32, lh32 = x32 - x32.floor(), y32 - y32.floor()
        lw64, lh64 = lw32.double(), lh32.double()
        for a32, b32, a64, b64 in ((1 - lh32, 1 - lw32, 1 - lh64, 1 - lw64), (1 - lh32, lw32, 1 - lh64, lw64),
                                   (lh32, 1 - lw32, lh64, 1 - lw64), (lh32, lw32, lh64, lw64)):
            assert bool(((a32 * b32).double() == a64 * b64).all())


# ---------------------------------------------------------------------------------------------------- float64 restatement
def _geom(loc_l, H, W):
    """One level, loc_l [..., 2] float64 (x, y): per corner (y0,x0) (y0,x1) (y1,x0) (y1,x1) the in-range mask, the pixel
    coordinates, the bilinear weight and its derivatives with respect to the pixel coordinates x and y (cuh:87-159)."""
    x = loc_l[..., 0] * W - 0.5
    y = loc_l[..., 1] * H - 0.5
    valid = (y > -1) & (x > -1) & (y < H) & (x < W)
    yf, xf = torch.floor(y), torch.floor(x)
    lh, lw = y - yf, x - xf
    hh, hw = 1 - lh, 1 - lw
    y0, x0 = yf.long(), xf.long()
    ys, xs = (y0, y0, y0 + 1, y0 + 1), (x0, x0 + 1, x0, x0 + 1)
    ok = tuple(valid & (ys[k] >= 0) & (ys[k] <= H - 1) & (xs[k] >= 0) & (xs[k] <= W - 1) for k in range(4))
    return ok, ys, xs, (hh * hw, hh * lw, lh * hw, lh * lw), (-hh, hh, -lh, lh), (-hw, -lw, hw, lw)


def _rows(B, S, Mh, pix):
    """Row of the [B * S * Mh, D] view of value for pixel index pix [B, Lq, Mh]."""
    base = torch.arange(B)[:, None, None] * (S * Mh) + torch.arange(Mh)[None, None, :]
    return (base + pix * Mh).reshape(-1)


def msda_forward_budget(value, shapes, lsi, loc, attn):
    """out [B, Lq, M*D] in float64 and the sum of |attn * w * value| over the terms of each element."""
    value, loc, attn = value.double(), loc.double(), attn.double()
    B, S, Mh, Dc = value.shape
    _, Lq, _, L, P, _ = loc.shape
    vflat = value.reshape(B * S * Mh, Dc)
    out = torch.zeros(B, Lq, Mh, Dc, dtype=F64)
    out_abs = torch.zeros_like(out)
    for l, (H, W) in enumerate(shapes):
        for p in range(P):
            ok, ys, xs, w, _, _ = _geom(loc[:, :, :, l, p, :], H, W)
            a = attn[:, :, :, l, p]
            for k in range(4):
                pix = int(lsi[l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1)
                t = (w[k] * a * ok[k].double())[..., None] * vflat[_rows(B, S, Mh, pix)].reshape(B, Lq, Mh, Dc)
                out += t
                out_abs += t.abs()
    return dict(out=out.reshape(B, Lq, Mh * Dc), abs_out=out_abs.reshape(B, Lq, Mh * Dc))


def msda_backward_budget(value, shapes, lsi, loc, attn, grad_out):
    """grad_value [B,S,M,D], grad_loc [B,Lq,M,L,P,2], grad_attn [B,Lq,M,L,P] in float64 from the given operands (widened
    exactly), with abs_grad_value / abs_grad_loc / abs_grad_attn = the sum of the absolute values of the added terms and
    n_terms = the number of nonzero contributions to each element of grad_value (int32)."""
    value, loc, attn = value.double(), loc.double(), attn.double()
    B, S, Mh, Dc = value.shape
    _, Lq, _, L, P, _ = loc.shape
    g = grad_out.double().reshape(B, Lq, Mh, Dc)
    vflat = value.reshape(B * S * Mh, Dc)
    gv = torch.zeros(B * S * Mh, Dc, dtype=F64)
    gv_abs = torch.zeros_like(gv)
    gv_n = torch.zeros(B * S * Mh, Dc, dtype=torch.int32)
    gl = torch.zeros(B, Lq, Mh, L, P, 2, dtype=F64)
    gl_abs = torch.zeros_like(gl)
    ga = torch.zeros(B, Lq, Mh, L, P, dtype=F64)
    ga_abs = torch.zeros_like(ga)
    for l, (H, W) in enumerate(shapes):
        assert int(lsi[l]) + H * W <= S
        for p in range(P):
            ok, ys, xs, w, dwx, dwy = _geom(loc[:, :, :, l, p, :], H, W)
            a = attn[:, :, :, l, p]
            for k in range(4):
                okf = ok[k].double()
                rows = _rows(B, S, Mh, int(lsi[l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1))
                # grad_value[corner] += w * attn * grad_out  (cuh:125-152)
                c = ((w[k] * a * okf)[..., None] * g).reshape(-1, Dc)
                gv.index_add_(0, rows, c)
                gv_abs.index_add_(0, rows, c.abs())
                gv_n.index_add_(0, rows, (c != 0).to(torch.int32))
                # d_k = <grad_out, value[corner]> over the channels; grad_attn = sum_k w_k d_k,
                # grad_loc.x = W * attn * sum_k (dw_k / dx) d_k, grad_loc.y likewise with H  (cuh:108-158)
                gvk = g * vflat[rows].reshape(B, Lq, Mh, Dc) * okf[..., None]
                d, d_abs = gvk.sum(-1), gvk.abs().sum(-1)
                ga[:, :, :, l, p] += w[k] * d
                ga_abs[:, :, :, l, p] += w[k] * d_abs
                gl[:, :, :, l, p, 0] += W * a * dwx[k] * d
                gl_abs[:, :, :, l, p, 0] += W * a.abs() * dwx[k].abs() * d_abs
                gl[:, :, :, l, p, 1] += H * a * dwy[k] * d
                gl_abs[:, :, :, l, p, 1] += H * a.abs() * dwy[k].abs() * d_abs
    shape = (B, S, Mh, Dc)
    return dict(grad_value=gv.reshape(shape), abs_grad_value=gv_abs.reshape(shape), n_terms=gv_n.reshape(shape),
                grad_loc=gl, abs_grad_loc=gl_abs, grad_attn=ga, abs_grad_attn=ga_abs)


# ------------------------------------------------------------------------------------------------------------ criteria
U = 2.0 ** -24   # unit roundoff of fp32


def worst_ratio(got, want, bound):
    """max |got - want| / bound; where the bound is 0 -- no term at all -- the result has to be exactly 0."""
    err = (got.double() - want).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an element without a contribution is not exactly 0"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def check_backward(label, got, ref, bf16=False, rows=None):
    """Element-wise criteria of an fp32 backward (got = grad_value, grad_loc, grad_attn) against msda_backward_budget's result:
    grad_value   (n_terms + 2) * 2^-24 * abs: one rounding for w * attn, one for * grad_out, one per addition, any order;
    grad_loc / grad_attn   32 * 2^-24 * abs: 4 multiply-adds, a 3-step 8-lane reduction and a 4-term combination are under
    16 roundings, 32 leaves a factor of two.
    bf16: the module rounds grad_value to bfloat16: 2^-8 |want| more for it.  rows: grad_loc / grad_attn of these queries only
    (ref was computed from them alone).  Prints and returns the worst ratio of error to bound of each gradient."""
    gv, gl, ga = (t.detach().cpu() for t in got)
    if rows is not None:
        gl, ga = gl[:, rows], ga[:, rows]
    bound_v = (ref["n_terms"].double() + 2) * U * ref["abs_grad_value"]
    if bf16:
        bound_v = bound_v + 2.0 ** -8 * ref["grad_value"].abs()
    ratios = dict(grad_value=worst_ratio(gv, ref["grad_value"], bound_v),
                  grad_loc=worst_ratio(gl, ref["grad_loc"], 32 * U * ref["abs_grad_loc"]),
                  grad_attn=worst_ratio(ga, ref["grad_attn"], 32 * U * ref["abs_grad_attn"]))
    print(f"{label}: worst error / bound  " + "  ".join(f"{n} {r:.4f}" for n, r in ratios.items()))
    for n, r in ratios.items():
        assert r <= 1.0, (label, n, r)
    return ratios


def check_forward(label, got, ref):
    """16 * 2^-24 * abs per element of the forward output."""
    r = worst_ratio(got.detach().cpu(), ref["out"], 16 * U * ref["abs_out"])
    print(f"{label}: worst error / bound  out {r:.4f}")
    assert r <= 1.0, (label, r)
    return r


# ------------------------------------------------------------------------------------- windows of the value-tile kernel
def tile_queries(shapes, lsi, Lq):
    """[ntiles, 64] query index of every slot of every tile, -1 = padding (msda_common.h: make_tile_map, tile_query).
    Encoder mode -- Lq equals the sum of the level sizes and the levels lie back to back -- tiles the levels in 8 x 8 pixel
    blocks, level 0 first; any other call takes 64 consecutive queries per tile."""
    grid2d = sum(h * w for h, w in shapes) == Lq and [int(s) for s in lsi] == level_starts(shapes)
    ql = np.arange(TQ * TQ)
    tiles = []
    if grid2d:
        for (H, W), st in zip(shapes, lsi):
            for ty in range(-(-H // TQ)):
                for tx in range(-(-W // TQ)):
                    qy, qx = ty * TQ + ql // TQ, tx * TQ + ql % TQ
                    tiles.append(np.where((qy < H) & (qx < W), int(st) + qy * W + qx, -1))
    else:
        for t in range(-(-Lq // (TQ * TQ))):
            q = t * TQ * TQ + ql
            tiles.append(np.where(q < Lq, q, -1))
    return np.stack(tiles)


def tile_windows(shapes, lsi, loc, Lq):
    """The bounding-box step of msda_bwd_value_tile_f32 for every (image, tile, head) item:
    rect [B, ntiles, M, L, 4] = (y0, y1, x0, x1) inclusive of the level window, (0, -1, 0, -1) where it is empty, and
    ntot [B, ntiles, M] = the sum of the window sizes = the length of the item's virtual pixel range.
    A valid sample -- one with any corner in range -- contributes the clamped corners max(y0, 0) .. min(y0 + 1, H - 1)
    and likewise in x, whatever their weights."""
    loc = loc.double().numpy()
    B, L = loc.shape[0], len(shapes)
    tq = tile_queries(shapes, lsi, Lq)
    big = 1 << 30
    rect = np.zeros((B, tq.shape[0], loc.shape[2], L, 4), dtype=np.int64)
    for l, (H, W) in enumerate(shapes):
        x, y = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5
        valid = (y > -1) & (x > -1) & (y < H) & (x < W)
        y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
        per_query = []
        for lo, hi in ((np.maximum(y0, 0), np.minimum(y0 + 1, H - 1)), (np.maximum(x0, 0), np.minimum(x0 + 1, W - 1))):
            per_query.append(np.where(valid, lo, big).min(-1))     # [B, Lq, M]
            per_query.append(np.where(valid, hi, -big).max(-1))
        for j, a in enumerate(per_query):
            pad = np.full((B, 1, a.shape[2]), big if j % 2 == 0 else -big, dtype=np.int64)
            a = np.concatenate([a, pad], 1)[:, tq, :]              # [B, ntiles, 64, M]; slot -1 -> the padding row
            rect[:, :, :, l, j] = a.min(2) if j % 2 == 0 else a.max(2)
    empty = rect[..., 0] > rect[..., 1]
    rect[empty] = (0, -1, 0, -1)
    ntot = ((rect[..., 1] - rect[..., 0] + 1) * (rect[..., 3] - rect[..., 2] + 1)).sum(-1)
    return dict(tiles=tq, rect=rect, ntot=ntot)


def item_of(b, tile, B, ntiles):
    """Index of (image b, tile) in a head's item list: item j = (image j % B, tile ntiles - 1 - j // B)."""
    return (ntiles - 1 - tile) * B + b


def item_at(j, B, ntiles):
    return j % B, ntiles - 1 - j // B


# ---------------------------------------------------------------------------------------------------------- case builders
def _cdiv(a, b):
    return -((-a) // b)


def _oob_k(rng, shape, size):
    """Grid indices whose pixel coordinate is <= -1 or >= size (both ends included: the comparisons of cuh:288 are strict)."""
    c = _cdiv(GRID // 2, size)
    d = rng.integers(c, GRID + 1, shape)
    return np.where(rng.random(shape) < 0.5, -d, GRID + d)


def _axis_k(rng, shape, size, p_oob=0.05, p_border=0.03):
    """Random grid indices along one axis of a level with `size` pixels: uniform over [0, 1], p_border in the strips
    (-1, 0) / (size - 1, size) where one corner column falls off, p_oob out of range (about 10 % of the samples over both axes)."""
    c = _cdiv(GRID // 2, size)
    k = rng.integers(0, GRID + 1, shape)
    u = rng.random(shape)
    strip = rng.integers(-c + 1, c, shape)
    k = np.where(u < p_border, np.where(rng.random(shape) < 0.5, strip, GRID - strip), k)
    return np.where(u > 1 - p_oob, _oob_k(rng, shape, size), k)


def _axis_place(rng, n, lo, hi, size):
    """n grid indices whose clamped corner range [max(x0, 0), min(x0 + 1, size - 1)] is inside [lo, hi]; the first reaches lo
    and the second hi.  x0 = -1 (only the upper corner in range) and x0 = size - 1 (only the lower) are used where the
    window touches the border, which is also the only way to a window one pixel wide."""
    allowed = list(range(lo, hi)) + ([-1] if lo == 0 else []) + ([size - 1] if hi == size - 1 else [])
    at_lo = [v for v in allowed if max(v, 0) == lo]
    at_hi = [v for v in allowed if min(v + 1, size - 1) == hi]
    assert n >= 2 and at_lo and at_hi, (lo, hi, size)
    x0 = rng.choice(np.asarray(allowed), n)
    x0[0], x0[1] = at_lo[0], at_hi[0]
    k_lo = np.where(x0 < 0, (-(GRID // 2)) // size + 1, -((-(2 * x0 + 1) * (GRID // 2)) // size))   # x > -1 is strict
    k_hi = -((-(2 * x0 + 3) * (GRID // 2)) // size) - 1
    assert (k_lo <= k_hi).all()
    return rng.integers(k_lo, k_hi + 1)


def place(k, rng, shapes, b, queries, head, l, rect, p_oob=0.1):
    """Overwrite the samples of level l of (image b, queries, head) in the grid-index array k [B, Lq, M, L, P, 2]: inside
    rect = (y0, y1, x0, x1), reaching all four sides, about p_oob of them out of range; rect None = all of them out of range."""
    H, W = shapes[l]
    queries = np.asarray(queries)
    n = len(queries) * k.shape[4]
    if rect is None:
        kx, ky = _oob_k(rng, n, W), _oob_k(rng, n, H)
    else:
        ky, kx = _axis_place(rng, n, rect[0], rect[1], H), _axis_place(rng, n, rect[2], rect[3], W)
        out = rng.random(n) < p_oob
        out[:2] = False
        kx = np.where(out, _oob_k(rng, n, W), kx)
    k[b, queries, head, l, :, 0] = kx.reshape(len(queries), -1)
    k[b, queries, head, l, :, 1] = ky.reshape(len(queries), -1)


def _finish(rng, k, shapes, lsi, S, grad_rows=None):
    B, Lq, Mh, L, P, _ = k.shape
    assert k.min() >= -GRID and k.max() <= 2 * GRID
    attn = rng.integers(0, 33, (B, Lq, Mh, L, P)) / 256.0
    grad_out = rng.integers(-256, 257, (B, Lq, Mh * D)) / 64.0
    if grad_rows is not None:
        keep = np.zeros(Lq, dtype=bool)
        keep[grad_rows] = True
        grad_out[:, ~keep] = 0.0
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    return dict(value=f32(rng.standard_normal((B, S, Mh, D))), shapes=torch.as_tensor(shapes, dtype=torch.long),
                lsi=torch.as_tensor(lsi, dtype=torch.long), loc=f32(k / float(GRID)), attn=f32(attn), grad_out=f32(grad_out),
                pyramid=[tuple(s) for s in shapes])


def random_grid_indices(rng, B, Lq, shapes):
    L = len(shapes)
    P = 16 // L
    k = np.empty((B, Lq, M, L, P, 2), dtype=np.int32)
    for l, (H, W) in enumerate(shapes):
        k[:, :, :, l, :, 0] = _axis_k(rng, (B, Lq, M, P), W)
        k[:, :, :, l, :, 1] = _axis_k(rng, (B, Lq, M, P), H)
    return k


def random_case(seed, B, shapes, Lq=None, lsi=None, S=None):
    """Seeded random operands on the grids of the module docstring (M = 8, D = 32, P = 16 / L)."""
    rng = np.random.default_rng(seed)
    lsi = level_starts(shapes) if lsi is None else list(lsi)
    S = sum(h * w for h, w in shapes) if S is None else S
    Lq = S if Lq is None else Lq
    return _finish(rng, random_grid_indices(rng, B, Lq, shapes), shapes, lsi, S)


SEAM_PYRAMID = [(32, 64), (16, 32), (8, 16), (4, 8)]      # S = 2720; 32 + 8 + 2 + 1 = 43 tiles per image
SEAM_B = 3                                                # 129 items per head, 32 workgroups per head


def _r(h, w, y0, x0):
    return (y0, y0 + h - 1, x0, x0 + w - 1)


_FULL = {l: (0, h - 1, 0, w - 1) for l, (h, w) in enumerate(SEAM_PYRAMID)}
# ntot -> level windows (levels not named are empty).  Two or more levels, so that a level's first column vb[l] lies inside a
# 32-column tile and inside a 448-column chunk; the level-0 widths 29, 41, 7, 6 do not divide 448, so the two rows of corners of
# one sample straddle chunk seams.
SEAM_WINDOWS = {
    1: {0: (0, 0, 0, 0)},
    31: {0: _r(3, 7, 5, 9), 1: _r(2, 5, 3, 4)},
    32: {0: _r(3, 6, 5, 9), 1: _r(2, 7, 3, 4)},
    33: {0: _r(3, 7, 5, 9), 1: _r(2, 3, 3, 4), 2: _r(2, 3, 1, 2)},
    447: {0: _r(15, 29, 10, 20), 1: _r(3, 4, 3, 4)},
    448: {0: _r(15, 29, 10, 20), 1: _r(13, 1, 2, 0)},        # 435 + a 13 x 1 window in column 0 of level 1
    449: {0: _r(15, 29, 10, 20), 1: _r(2, 7, 3, 4)},
    895: {0: _r(21, 41, 5, 11), 1: _r(2, 17, 3, 4)},
    896: {0: _r(21, 41, 5, 11), 1: _r(5, 7, 3, 4)},
    897: {0: _r(21, 41, 5, 11), 1: _r(4, 9, 3, 4)},
    2720: _FULL,
}
# Workgroup w of a head starts with items w and 32 + w of that head (msda_tile.hip: "w, npx + w") and draws the rest from the
# counter.  Head h gets its two targets on workgroup h: SEAM_FIRST[h] on item h, SEAM_SECOND[h] on item 32 + h.  On heads 0, 1, 2
# and 7 a small window therefore follows a larger one on the same workgroup (1 after 2720, 31 after 897, 32 after 896, 1 after
# 33): the columns the large item filled must have been zeroed again.  On head 6 the full window follows a 447-column one.
SEAM_FIRST = [2720, 897, 896, 895, 449, 448, 447, 33]
SEAM_SECOND = [1, 31, 32, 447, 448, 449, 2720, 1]


def _window_size(win):
    return sum((r[1] - r[0] + 1) * (r[3] - r[2] + 1) for r in win.values())


def _place_item(k, rng, shapes, tq, b, tile, head, win):
    queries = tq[tile][tq[tile] >= 0]
    for l in range(len(shapes)):
        place(k, rng, shapes, b, queries, head, l, win.get(l))


def seams_case(seed=101):
    """Selected (image, tile, head) items with prescribed window sizes; `expect` maps (b, tile, head) -> ntot."""
    rng = np.random.default_rng(seed)
    shapes, B = SEAM_PYRAMID, SEAM_B
    lsi, S = level_starts(shapes), sum(h * w for h, w in shapes)
    tq = tile_queries(shapes, lsi, S)
    k = random_grid_indices(rng, B, S, shapes)
    expect = {}
    for head in range(M):
        for j, target in ((head, SEAM_FIRST[head]), (NPX + head, SEAM_SECOND[head])):
            assert _window_size(SEAM_WINDOWS[target]) == target
            b, tile = item_at(j, B, tq.shape[0])
            _place_item(k, rng, shapes, tq, b, tile, head, SEAM_WINDOWS[target])
            expect[(b, tile, head)] = target
    x = _finish(rng, k, shapes, lsi, S)
    x["expect"] = expect
    return x


def empty_case(seed=102):
    """Image 0, tile 10: level 0 empty for every head.  Head 3, item 1 (the first item of workgroup 1, followed there by
    item 33) and head 5, item 34 (the second item of workgroup 2, followed by a counter-drawn one): no sample in range at all,
    ntot = 0.  Everything around them is ordinary."""
    rng = np.random.default_rng(seed)
    shapes, B = SEAM_PYRAMID, SEAM_B
    lsi, S = level_starts(shapes), sum(h * w for h, w in shapes)
    tq = tile_queries(shapes, lsi, S)
    k = random_grid_indices(rng, B, S, shapes)
    for head in range(M):
        place(k, rng, shapes, 0, tq[10][tq[10] >= 0], head, 0, None)
    expect = {}
    for head, j in ((3, 1), (5, NPX + 2)):
        b, tile = item_at(j, B, tq.shape[0])
        _place_item(k, rng, shapes, tq, b, tile, head, {})
        expect[(b, tile, head)] = 0
    x = _finish(rng, k, shapes, lsi, S)
    x["expect"], x["empty_level0"] = expect, (0, 10)
    return x


DEGENERATE_PYRAMID = [(17, 16), (1, 9), (9, 1), (1, 1)]   # S = 291


def big_case(seed, shapes):
    """B = 1 at and beyond 65 536 pixels.  The queries of the first, a middle and the last tile sample every level from corner to
    corner for every head (their windows are the whole levels: ntot = S) and are the only ones with a nonzero grad_out; every
    other query samples within two pixels of its own position.  `rows` lists those queries."""
    rng = np.random.default_rng(seed)
    L = len(shapes)
    P = 16 // L
    lsi, S = level_starts(shapes), sum(h * w for h, w in shapes)
    tq = tile_queries(shapes, lsi, S)
    k = np.empty((1, S, M, L, P, 2), dtype=np.int32)
    for (Hq, Wq), st in zip(shapes, lsi):
        q = np.arange(Hq * Wq)
        cy, cx = ((q // Wq + 0.5) / Hq)[:, None, None], ((q % Wq + 0.5) / Wq)[:, None, None]
        for l, (H, W) in enumerate(shapes):
            dx, dy = rng.uniform(-2, 2, (Hq * Wq, M, P)), rng.uniform(-2, 2, (Hq * Wq, M, P))
            k[0, st:st + Hq * Wq, :, l, :, 0] = np.clip(np.rint((cx + dx / W) * GRID), -GRID, 2 * GRID)
            k[0, st:st + Hq * Wq, :, l, :, 1] = np.clip(np.rint((cy + dy / H) * GRID), -GRID, 2 * GRID)
    chosen = [0, tq.shape[0] // 2, tq.shape[0] - 1]
    full = {l: (0, h - 1, 0, w - 1) for l, (h, w) in enumerate(shapes)}
    for tile in chosen:
        for head in range(M):
            _place_item(k, rng, shapes, tq, 0, tile, head, full)
    rows = np.concatenate([tq[t][tq[t] >= 0] for t in chosen])
    x = _finish(rng, k, shapes, lsi, S, grad_rows=rows)
    x["rows"], x["chosen_tiles"] = torch.from_numpy(rows), chosen
    return x


BIG_ONE_LEVEL = [(257, 256)]                                   # S = 65 792: one level beyond 16 bits
BIG_PYRAMID = [(200, 200), (150, 150), (64, 64), (16, 16)]     # S = 66 852: no single level is, only the sum

CASES = {
    "seams": seams_case,
    "empty": empty_case,
    "degenerate": lambda: random_case(103, 2, DEGENERATE_PYRAMID),
    "l1_tile": lambda: random_case(104, 2, [(16, 16)]),                       # Lq = S = 256: the tile pair
    "l1_split4": lambda: random_case(105, 2, [(16, 16)], Lq=40),              # four waves per query
    "l1_split1": lambda: random_case(106, 1, [(16, 16)], Lq=5000),            # one wave per query, with its atomics
    "gapped": lambda: random_case(107, 2, [(16, 16), (8, 8)], lsi=[0, 261], S=325),
}
BOUNDARY_CASE = lambda: big_case(110, [(256, 256)])             # noqa: E731  S = 65 536: ids up to 65 535, the last that fit
BIG_CASES = {
    "big_one_level": lambda: big_case(108, BIG_ONE_LEVEL),
    "big_pyramid": lambda: big_case(109, BIG_PYRAMID),
}
