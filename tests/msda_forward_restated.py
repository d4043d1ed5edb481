"""Float64 restatement of the FUSED MSDA forward (prologue + gather) with error budgets, operands for which every forward kernel
is exact, and the constructed cases of tests/test_gpu_msda_forward_edges.py.  CPU only; calls neither oracle/msda.py nor any
kernel (tests/test_msda_forward_cases_cpu.py compares it with the oracle and checks that each case is what it is named for).

Exact grid.  Pyramids with power-of-two sides; reference points on multiples of 1 / (4 Wg), Wg = min(W, 32), in about
[-1/8, 9/8] (at most 8 significant bits: bfloat16-exact); offsets on multiples of 1/4 pixel below 64 pixels (bfloat16-exact).
1 / W is a power of two, so ``ref + off * (1 / W)`` and ``ref + off / W`` are the same exact fp32 number, pixel coordinates have
quarter-pixel fractions, the four bilinear weights are k / 16, and with logits 0 on n selected slots and -1024 elsewhere
(n a power of two; exp(-1024) underflows to exactly 0 in fp32 and float64) the attention is exactly 1 / n on the selected slots:
weight x attention is k / (16 n), bfloat16-exact for n <= 16.  Values are integers in [-7, 7], the value bias integers in
[-3, 3]: every term and every partial sum is a multiple of 2^-8 far below 2^15, so an fp32 kernel must return the float64
result bit for bit, in any order of addition, and a bf16 kernel its round-to-nearest-even bfloat16 image.  4-d boxes carry
wh = 2 P 2^j / (W, H), j in {0, 1}: ``off / P * wh * 0.5 = off 2^j / W``, on the same grid.  ``assert_exact_forward`` checks a case
against all of this directly instead of trusting the argument.

Budgets off the grid (``bound_f32`` / ``bound_bf16``; u = 2^-24, abs = sum of |attn w value| over the terms of an element):
  fp32   16 u abs (check_forward of msda_restated.py)  +  (63 + 2) u |bias| sum |attn w|: the kernel adds the 64 corner weights
         (63 additions), multiplies by the bias and adds the product -- one rounding each;
  bf16   (2^-8 + 80 u) abs + 2^-8 |out|: 2^-8 is the unit roundoff of bfloat16, paid once for the corner weight rounded for the
         dot instruction and once for the rounded output; 80 u covers the 64 fp32 accumulations and the weight's own roundings;
  geometry (fused entries, arbitrary pyramids): the kernel forms the location in fp32.  Point form, reciprocal order:
         iw = rn(1 / W) = (1 + e1) / W, t = rn(off iw), loc = rn(ref + t), then x = rn(rn(loc W) - 0.5) (or one fused rounding),
         |e| <= u each, so in pixels |x - x*| <= W (2 u |off| / W + u |loc*|) + u W |loc*| + u |x*| <= u (3 W |loc*| + 2 |off| + 1/2)
         to first order (the division order has one rounding fewer).  Box form: t = rn(rn(off / P) wh) 0.5 has the same two
         roundings on the displacement d = W |off / P wh / 2| pixels.  delta = 1.001 u (3 W |loc*| + 2 d + 1) bounds both, with
         room for the second-order terms.  The forward is continuous and, inside one pixel cell, linear in x and in y, so the
         location error costs at most  sum_k attn |v_k| (|dw_k / dx| delta_x + |dw_k / dy| delta_y)  -- provided no sample lies
         within 2 delta of a cell boundary, which ``odd_fused_case`` arranges and ``geometry_delta`` asserts.  The roundings of hh = 1 - lh,
         hw = 1 - lw and of their product get no term of their own: they stay inside the 16 u abs.
"""
import functools

import numpy as np
import torch

import msda_restated as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = R.U
UB = 2.0 ** -8        # unit roundoff of bfloat16
M, D = R.M, R.D
NEG = -1024.0         # logit of an unselected slot
P2 = [(16, 32), (8, 16), (4, 8), (2, 4)]     # S = 680
HUGE = 2.0 ** 100     # about 1.27e30, bfloat16-exact
ONE = [(1, 1)] * 4


# ------------------------------------------------------------------------------------------------------------- prologue
def _sizes(x, dtype):
    sh = x["shapes"].to(dtype)
    return sh[:, 1].view(1, 1, 1, -1, 1), sh[:, 0].view(1, 1, 1, -1, 1)     # W, H broadcast over [B, Lq, M, L, P]


def locations(x, form, dtype=F64, order="div", neighbour_w=False):
    """loc [B, Lq, M, L, P, 2] of the fused prologue (model source deformable_detr.py:1055-1081) in `dtype`:
    point: ref + off / (W, H) (order "div") or ref + off * (1 / (W, H)) ("rcp", the kernels'); box: ref.xy + off / P * wh * 0.5."""
    off = x["off"].to(dtype)
    W, H = _sizes(x, dtype)
    if neighbour_w:    # mutation: the W of the next level
        W = W.roll(-1, 3)
    ref = x["ref"].to(dtype)[:, :, None, :, None, :]
    if form == "box":
        wh = x["boxwh"].to(dtype)[:, :, None, :, None, :]
        return ref + off / float(off.shape[4]) * wh * 0.5
    n = torch.stack([W.expand(off.shape[:-1]), H.expand(off.shape[:-1])], -1)
    return ref + (off / n if order == "div" else off * (1.0 / n))


def attention(x, dtype=F64):
    """softmax over the L * P logits of a head, [B, Lq, M, L, P]."""
    lg = x["logit"].to(dtype)
    e = torch.exp(lg - lg.max(-1, keepdim=True).values)
    return (e / e.sum(-1, keepdim=True)).reshape(x["off"].shape[:-1])


def sane(loc):
    """A NaN coordinate fails every range comparison of the kernel (msda_common.h: valid == false): the sample is out of range
    like any other.  The float64 geometry below would carry the NaN into 0 * NaN, so it is moved to -4."""
    return torch.where(torch.isnan(loc), torch.full_like(loc, -4.0), loc)


# ---------------------------------------------------------------------------------------------------------- accumulation
def accumulate(value, shapes, lsi, loc, attn, drop=None, delta=None):
    """msda_forward_budget (msda_restated.py) again with two hooks: drop = (slot, corner) leaves that corner out (a mutation),
    delta = (dx, dy) [B, Lq, M, L, P] in pixels returns the geometry term of the module docstring as `geo`."""
    value, loc, attn = value.double(), loc.double(), attn.double()
    B, S, Mh, Dc = value.shape
    _, Lq, _, L, P, _ = loc.shape
    vflat = value.reshape(B * S * Mh, Dc)
    out = torch.zeros(B, Lq, Mh, Dc, dtype=F64)
    out_abs, geo = torch.zeros_like(out), torch.zeros_like(out)
    for l, (H, W) in enumerate(shapes):
        for p in range(P):
            ok, ys, xs, w, dwx, dwy = R._geom(loc[:, :, :, l, p, :], H, W)
            a = attn[:, :, :, l, p]
            for k in range(4):
                if drop == (l * P + p, k):
                    continue
                pix = int(lsi[l]) + ys[k].clamp(0, H - 1) * W + xs[k].clamp(0, W - 1)
                v = vflat[R._rows(B, S, Mh, pix)].reshape(B, Lq, Mh, Dc)
                okf = ok[k].double()
                t = (w[k] * a * okf)[..., None] * v
                out += t
                out_abs += t.abs()
                if delta is not None:
                    g = a.abs() * okf * (dwx[k].abs() * delta[0][:, :, :, l, p] + dwy[k].abs() * delta[1][:, :, :, l, p])
                    geo += g[..., None] * v.abs()
    r = lambda t: t.reshape(B, Lq, Mh * Dc)  # noqa: E731
    return dict(out=r(out), abs_out=r(out_abs), geo=r(geo))


def geometry_delta(x, form):
    """(dx, dy) in pixels per sample, the delta of the module docstring; asserts that no finite in-range sample lies within
    2 delta of a pixel-cell boundary."""
    loc = sane(locations(x, form))
    W, H = _sizes(x, F64)
    off = torch.nan_to_num(x["off"].double(), nan=0.0)
    if form == "box":
        disp = (off / off.shape[4] * x["boxwh"].double()[:, :, None, :, None, :] * 0.5).abs()
        disp = torch.stack([disp[..., 0] * W, disp[..., 1] * H], -1)
    else:
        disp = off.abs()
    out = []
    for c, n in ((0, W), (1, H)):
        d = 1.001 * U * (3 * n * loc[..., c].abs() + 2 * disp[..., c] + 1)
        pix = loc[..., c] * n - 0.5
        near = (pix - pix.round()).abs() <= 2 * d
        assert not bool((near & (pix > -2) & (pix < n + 1)).any()), "a sample within 2 delta of a pixel-cell boundary"
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------- reference
MUTATIONS = ("drop_corner", "neighbour_slot", "other_image_mask", "next_bit", "neighbour_w", "dead_half", "bias_on_padded")


def applies(x, mut):
    """Whether a mutation can change anything in a case at all: the mask mutations need a second image / a mask, the level
    mutation two levels of different width, the half mix-up of the last bf16 pair an odd number of queries."""
    B, Lq = x["off"].shape[:2]
    if mut == "other_image_mask":
        return B >= 2
    if mut == "neighbour_w":
        return len({w for _, w in x["pyramid"]}) >= 2
    if mut == "dead_half":
        return (B * Lq) % 2 == 1 and B * Lq >= 3
    return True


def reference(x, form="point", mask=False, bias=False, mut=None, geometry=False):
    """The fused forward in float64.  out, abs_out (value terms), abs_bias (|bias| sum |attn w| over unpadded in-range corners),
    geo (0 unless geometry=True) and weights (the softmax).  mask: rows of padded tokens are zero and get no bias
    (deformable_detr.py:1048-1052).  mut: one of MUTATIONS, a deliberately wrong restatement for the CPU tests."""
    B, Lq = x["off"].shape[:2]
    loc = sane(locations(x, form, neighbour_w=mut == "neighbour_w"))
    attn = attention(x)
    keep = x["keep"] if mask else torch.ones_like(x["keep"])
    if mut == "other_image_mask":
        keep = keep.roll(1, 0)
    if mut == "next_bit":
        keep = keep.roll(-1, 1)
    if mut == "neighbour_slot":          # one slot gathers with the record of the next slot (of a level of the same size)
        L, P = loc.shape[3:5]
        loc, attn = loc.clone().flatten(3, 4), attn.clone().flatten(3, 4)
        a, b = (3, 4) if tuple(x["pyramid"][3 // P]) == tuple(x["pyramid"][4 // P]) else (2, 3)
        loc[:, :, :, a], attn[:, :, :, a] = loc[:, :, :, b], attn[:, :, :, b]
        loc, attn = loc.unflatten(3, (L, P)), attn.unflatten(3, (L, P))
    # dead_half: the last query gathers with the records of the query before it -- a mix-up of the two halves of the last bf16
    # pair.  It shows that the criteria notice a wrong record there; it is NOT the kernel's missing clamp: the dead half
    # (q = nq_total, clamped to nq_total - 1) never stores, so without the clamp the kernel would read out of range, not
    # return a wrong output, and no test provokes that.
    if mut == "dead_half":
        loc, attn = loc.clone().flatten(0, 1), attn.clone().flatten(0, 1)
        loc[-1], attn[-1] = loc[-2], attn[-2]
        loc, attn = loc.unflatten(0, (B, Lq)), attn.unflatten(0, (B, Lq))
    kf = keep.double()[:, :, None, None]
    value = x["value"].double() * kf
    shapes, lsi = x["pyramid"], x["lsi"].tolist()
    delta = geometry_delta(x, form) if geometry else None
    if mut is None and delta is None:
        r = R.msda_forward_budget(value, shapes, lsi, loc, attn)
        r["geo"] = torch.zeros_like(r["out"])
    else:
        r = accumulate(value, shapes, lsi, loc, attn, drop=(5, 3) if mut == "drop_corner" else None, delta=delta)
    r["abs_bias"] = torch.zeros_like(r["out"])
    r["out_nobias"], r["geo_nobias"] = r["out"], r["geo"]
    if bias:
        ones = torch.ones(B, x["value"].shape[1], M, 1, dtype=F64)
        ws = accumulate(ones if mut == "bias_on_padded" else ones * kf, shapes, lsi, loc, attn, delta=delta)
        vb = x["vbias"].double().view(1, 1, M, D)
        rep = lambda t: t.reshape(B, Lq, M, 1)  # noqa: E731
        r["out"] = r["out"] + (rep(ws["out"]) * vb).reshape(B, Lq, M * D)
        r["abs_bias"] = (rep(ws["abs_out"]) * vb.abs()).reshape(B, Lq, M * D)
        r["geo"] = r["geo"] + (rep(ws["geo"]) * vb.abs()).reshape(B, Lq, M * D)
    r["weights"] = attention(x)
    return r


def bound_f32(r):
    return 16 * U * r["abs_out"] + 65 * U * r["abs_bias"] + r["geo"]


def bound_bf16(r):
    return (UB + 80 * U) * (r["abs_out"] + r["abs_bias"]) + UB * r["out"].abs() + r["geo"]


def check(label, got, r, bound):
    ratio = R.worst_ratio(got.detach().cpu(), r["out"], bound)
    print(f"{label}: worst error / bound  out {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)
    return ratio


def without_bias(r):
    """The reference of the same call without a value bias, from one made with it."""
    return dict(r, out=r["out_nobias"], geo=r["geo_nobias"], abs_bias=torch.zeros_like(r["out"]))


def plain_operands(x, form="point"):
    """loc / attn of the plain entries: the prologue evaluated in fp32 (for an exact case this IS the float64 value; NaN and
    huge locations are handed on as they are)."""
    return locations(x, form, F32, "rcp").contiguous(), attention(x, F32).contiguous()


# --------------------------------------------------------------------------------------------------- precondition checker
def _same(a, b):
    return bool(((a.double() == b.double()) | (torch.isnan(a) & torch.isnan(b))).all())


def _bf16_exact(t):
    t = t[torch.isfinite(t)]
    return bool((t.to(BF).double() == t.double()).all())


def assert_exact_forward(x):
    """The conditions of the module docstring and their consequences, checked directly on a case."""
    n = x["n"]
    assert n in (1, 2, 4, 8, 16)
    for name in ("value", "ref", "off", "logit", "vbias"):
        assert x[name].dtype == F32 and _bf16_exact(x[name]), name
    for form in ("point", "box"):
        loc64 = locations(x, form)
        for order in ("rcp", "div"):
            loc32 = locations(x, form, F32, order)
            assert loc32.dtype == F32 and _same(loc32, loc64), (form, order)
        loc32, loc64 = sane(locations(x, form, F32)), sane(loc64)
        for l, (H, W) in enumerate(x["pyramid"]):
            for c, size in ((0, W), (1, H)):       # loc * size - 0.5: exact unfused, therefore exact fused as well
                p32 = loc32[:, :, :, l, :, c] * float(size)
                assert _same(p32, loc64[:, :, :, l, :, c] * size) and _same(p32 - 0.5, loc64[:, :, :, l, :, c] * size - 0.5)
            ok, _, _, w64, _, _ = R._geom(loc64[:, :, :, l], H, W)
            x32, y32 = loc32[:, :, :, l, :, 0] * float(W) - 0.5, loc32[:, :, :, l, :, 1] * float(H) - 0.5
            lw, lh = x32 - x32.floor(), y32 - y32.floor()
            a64 = attention(x)[:, :, :, l]
            for k, w32 in enumerate(((1 - lh) * (1 - lw), (1 - lh) * lw, lh * (1 - lw), lh * lw)):
                inr = ok[k]
                assert w32.dtype == F32 and _same(w32[inr], w64[k][inr])
                wa = (w64[k] * a64)[inr]
                assert _bf16_exact(wa) and bool(((wa * 256) == (wa * 256).round()).all())
    a32, a64 = attention(x, F32), attention(x)
    assert _same(a32, a64)
    sel = x["logit"].reshape(a64.shape) == 0
    assert bool((sel.flatten(3).sum(-1) == n).all()) and bool((a64[sel] == 1.0 / n).all()) and bool((a64[~sel] == 0).all())
    for form, mask, bias in (("point", False, False), ("point", True, True), ("box", True, True)):
        r = reference(x, form, mask, bias)
        assert float((r["abs_out"] + r["abs_bias"]).max()) < 2.0 ** 15
        assert bool((r["out"] * 256 == (r["out"] * 256).round()).all())
        if n <= 2 and not bias:
            assert _bf16_exact(r["out"])


# ---------------------------------------------------------------------------------------------------------- case builders
def _wg(size):
    return min(size, 32)


class _Builder:
    def __init__(self, seed, pyramid, B, Lq, n, select):
        self.rng = rng = np.random.default_rng(seed)
        self.pyramid, self.B, self.Lq, self.n = [tuple(s) for s in pyramid], B, Lq, n
        self.L = L = len(pyramid)
        self.P = P = 16 // L
        self.S = sum(h * w for h, w in pyramid)
        self.k = np.zeros((B, Lq, L, 2), dtype=np.int64)          # ref = k / (4 Wg)
        self.j = np.zeros((B, Lq, M, L, P, 2), dtype=np.float64)  # off = j / 4 pixels
        for l, (H, W) in enumerate(pyramid):
            for c, size in ((0, W), (1, H)):
                g, half = _wg(size), -(-_wg(size) // 2)
                self.k[:, :, l, c] = rng.integers(-half, 4 * g + half + 1, (B, Lq))
                jm = min(max(size, 2), 32)
                self.j[:, :, :, l, :, c] = rng.integers(-jm, jm + 1, (B, Lq, M, P))
        self.boxj = rng.integers(0, 2, (B, Lq, L))
        i = np.arange(B * Lq).reshape(B, Lq, 1)
        if select == "slots":
            slot = (i + np.arange(M)[None, None, :]) % 16
            self.sel = np.arange(16)[None, None, None, :] == slot[..., None]
        else:
            self.sel = np.argsort(rng.random((B, Lq, M, 16)), -1) < n
        self.value = rng.integers(-7, 8, (B, self.S, M, D), dtype=np.int8)
        self.vbias = rng.integers(-3, 4, M * D)
        self.keep = rng.random((B, self.S)) < 0.5
        for b in range(B):      # token 0 and token S - 1 differ between neighbouring images
            self.keep[b, 0], self.keep[b, -1] = b % 2 == 0, b % 2 == 1
        self.placed, self.levels_used = set(), set()

    def put(self, b, q, h, slot, px, py):
        """Move the sample to pixel coordinates (px, py) (multiples of 1/4, or NaN / +-HUGE) by its offset; the box of that
        (query, level) gets j = 0 so that the box form lands on the same place."""
        l, p = divmod(slot, self.P)
        H, W = self.pyramid[l]
        for c, (size, t) in enumerate(((W, px), (H, py))):
            if not np.isfinite(t) or abs(t) >= HUGE:
                self.j[b, q, h, l, p, c] = t * 4
                continue
            mult = size // _wg(size)
            if abs(4 * t + 2 - self.k[b, q, l, c] * mult) > 128:   # wide levels: the reference point comes along, so that the
                assert (b, q, l) not in self.levels_used               # offset stays bfloat16-exact (first placement of the query only)
                self.k[b, q, l, c] = int(round((4 * t + 2) / mult))
            self.j[b, q, h, l, p, c] = 4 * t + 2 - self.k[b, q, l, c] * mult
        self.boxj[b, q, l] = 0
        self.placed.add((b, q, h))
        self.levels_used.add((b, q, l))

    def select_only(self, b, q, h, slot):
        self.sel[b, q, h] = False
        self.sel[b, q, h, slot] = True

    def touch_end_tokens(self):
        """Per image one selected sample exactly on token 0 and one exactly on token S - 1 (weight 1 on that corner)."""
        Hl, Wl = self.pyramid[-1]
        for b in range(self.B):
            for lvl, px, py in ((0, 0.0, 0.0), (self.L - 1, Wl - 1.0, Hl - 1.0)):
                done = False
                for q in range(self.Lq - 1, -1, -1):
                    for h in range(M):
                        slots = [s for s in np.flatnonzero(self.sel[b, q, h]) if s // self.P == lvl]
                        if slots and (b, q, h) not in self.placed and not done:
                            self.put(b, q, h, int(slots[0]), px, py)
                            done = True
                assert done, "no selected sample on the level"

    def finish(self, name, plant=False):
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
        B, Lq, L, P = self.B, self.Lq, self.L, self.P
        ref = np.zeros((B, Lq, L, 2))
        wh = np.zeros((B, Lq, L, 2))
        for l, (H, W) in enumerate(self.pyramid):
            for c, size in ((0, W), (1, H)):
                ref[:, :, l, c] = self.k[:, :, l, c] / (4.0 * _wg(size))
                wh[:, :, l, c] = 2.0 * P * 2.0 ** self.boxj[:, :, l] / size
        x = dict(name=name, n=self.n, pyramid=self.pyramid, exact=True, value=f32(self.value), vbias=f32(self.vbias),
                 shapes=torch.as_tensor(self.pyramid, dtype=torch.long),
                 lsi=torch.as_tensor(R.level_starts(self.pyramid), dtype=torch.long),
                 ref=f32(ref), boxwh=f32(wh), off=f32(self.j / 4.0), keep=torch.from_numpy(self.keep.copy()),
                 logit=f32(np.where(self.sel, 0.0, NEG)))
        if plant:
            _plant_masked_corners(x)
        return x


def _plant_masked_corners(x):
    """On every level, the token under one in-range corner with a nonzero weight of one selected sample becomes padding."""
    loc, sel = sane(locations(x, "point")), (x["logit"] == 0).reshape(x["off"].shape[:-1])
    S = x["keep"].shape[1]
    for l, (H, W) in enumerate(x["pyramid"]):
        ok, ys, xs, w, _, _ = R._geom(loc[:, :, :, l], H, W)
        pix = int(x["lsi"][l]) + ys[0].clamp(0, H - 1) * W + xs[0].clamp(0, W - 1)
        cand = (ok[0] & (w[0] > 0) & sel[:, :, :, l] & (pix != 0) & (pix != S - 1)).nonzero()
        assert len(cand), "no in-range corner to mask on the level"
        b, q, h, p = cand[0].tolist()
        x["keep"][b, int(pix[b, q, h, p])] = False


def grid_case(name, seed, pyramid, B, Lq, n, select="random", plant=False):
    bld = _Builder(seed, pyramid, B, Lq, n, select)
    bld.touch_end_tokens()
    return bld.finish(name, plant)


def _fall(size):
    """Pixel coordinates with x0 = -1, x0 = 0 (inside: both corners in range) and x0 = size - 1."""
    return (-0.75, 0.25, size - 0.5)


def falloff_placements():
    """(level, x, y): the nine combinations of {x0 = -1, inside, x0 = W - 1} x {the same in y} on every level, the four
    coordinates exactly -1 / W / H (strictly outside), and NaN / +-HUGE locations."""
    out = []
    for l, (H, W) in enumerate(P2):
        out += [(l, px, py) for px in _fall(W) for py in _fall(H)]
        out += [(l, -1.0, 0.25), (l, float(W), 0.25), (l, 0.25, -1.0), (l, 0.25, float(H))]
    return out + [(0, float("nan"), 0.25), (1, 0.25, float("nan")), (2, HUGE, 0.25), (3, 0.25, -HUGE), (0, float("nan"), float("nan"))]


def one_case(seed=212):
    """Four 1 x 1 levels, one query: slot 5 of head 2 sits at x0 = y0 = -1, where (y1, x1) is the only corner in range."""
    bld = _Builder(seed, ONE, 1, 1, 16, "random")
    bld.put(0, 0, 2, 5, -0.75, -0.75)
    bld.touch_end_tokens()
    return bld.finish("one")


def falloff_case(seed=207):
    bld = _Builder(seed, P2, 2, 64, 1, "slots")
    for t, (l, px, py) in enumerate(falloff_placements()):
        i, h = divmod(t, M)
        b, q = divmod(i, bld.Lq)
        slot = l * bld.P + t % bld.P
        bld.select_only(b, q, h, slot)
        bld.put(b, q, h, slot, px, py)
    bld.touch_end_tokens()
    return bld.finish("falloff", plant=True)


def _nudge_off_cell_boundaries(x):
    """Offsets (bfloat16-exact before and after) are moved until no in-range sample of either form lies within 2^-10 pixel of a
    pixel-cell boundary: inside a cell the forward is linear in the location (the premise of the geometry term)."""
    W, H = _sizes(x, F64)
    for it in range(1, 40):
        near = torch.zeros(x["off"].shape, dtype=torch.bool)
        for form in ("point", "box"):
            loc = locations(x, form)
            for c, n in ((0, W), (1, H)):
                pix = loc[..., c] * n - 0.5
                near[..., c] |= ((pix - pix.round()).abs() < 2.0 ** -10) & (pix > -2) & (pix < n + 1)
        if not bool(near.any()):
            return
        x["off"] = torch.where(near, (x["off"] + 0.03125 * it).to(BF).float(), x["off"])
    raise AssertionError("samples stay on cell boundaries")


def odd_fused_case(name, seed, pyramid, B, Lq):
    """Budget case of the fused entries on an arbitrary pyramid: full-mantissa bfloat16-representable reference points, offsets,
    boxes, values (so that the fp32 and the bf16 entries take the same operands), exact logits (n = 8: the softmax stays exact
    and the case pays the geometry term alone), fp32 value bias."""
    g = torch.Generator().manual_seed(seed)
    pyramid = [tuple(s) for s in pyramid]
    L = len(pyramid)
    P = 16 // L
    S = sum(h * w for h, w in pyramid)
    rb = lambda t: t.to(BF).float()  # noqa: E731
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    sel = torch.argsort(torch.rand(B, Lq, M, 16, generator=g), -1) < 8
    keep = torch.rand(B, S, generator=g) < 0.5
    for b in range(B):
        keep[b, 0], keep[b, -1] = b % 2 == 0, b % 2 == 1
    sizes = torch.tensor([[w, h] for h, w in pyramid], dtype=F32)
    x = dict(name=name, n=8, pyramid=pyramid, exact=False, value=rb(rnd(B, S, M, D)), vbias=0.25 * rnd(M * D),
             shapes=torch.as_tensor(pyramid, dtype=torch.long), lsi=torch.as_tensor(R.level_starts(pyramid), dtype=torch.long),
             ref=rb(torch.rand(B, Lq, L, 2, generator=g) * 1.2 - 0.1),
             boxwh=rb((0.5 + torch.rand(B, Lq, L, 2, generator=g)) * 2.0 * P / sizes),
             off=rb(1.5 * rnd(B, Lq, M, L, P, 2)), keep=keep, logit=torch.where(sel, 0.0, NEG).float())
    _nudge_off_cell_boundaries(x)
    return x


def containment_rows(x, form, b, pixel):
    """[Lq, M] bool: the (query, head) rows of image b whose 16 records have `pixel` (a token index) among their four clamped
    corner addresses -- msda_common.h sample_geom: an invalid sample takes (y0, x0) = (0, 0), and every record is read whatever
    its weights: masked, unselected and out-of-range corners too."""
    loc = sane(locations(x, form))[b]
    hit = torch.zeros(loc.shape[:2], dtype=torch.bool)
    for l, (H, W) in enumerate(x["pyramid"]):
        px, py = loc[:, :, l, :, 0] * W - 0.5, loc[:, :, l, :, 1] * H - 0.5
        valid = (py > -1) & (px > -1) & (py < H) & (px < W)
        y0 = torch.where(valid, py.floor(), torch.zeros_like(py)).long()
        x0 = torch.where(valid, px.floor(), torch.zeros_like(px)).long()
        for yy in (y0.clamp(min=0), (y0 + 1).clamp(max=H - 1)):
            for xx in (x0.clamp(min=0), (x0 + 1).clamp(max=W - 1)):
                hit |= ((int(x["lsi"][l]) + yy * W + xx) == pixel).any(-1)
    return hit


BITS_LAST_LDS = [(128, 128), (64, 128), (64, 64), (32, 128)]      # S = 32 768: 1024 mask words, the last size staged in LDS
BITS_MEMORY = [(128, 256), (8, 16), (4, 8), (2, 4)]               # S = 32 936: 1030 words, bits read from memory
ODD = [(19, 31), (10, 16), (5, 8), (3, 4)]

EXACT_CASES = {
    "slots": lambda: grid_case("slots", 201, P2, 3, 37, 1, "slots", plant=True),
    "slots_wave": lambda: grid_case("slots_wave", 202, P2, 2, 515, 1, "slots"),
    "threshold_1024": lambda: grid_case("threshold_1024", 203, P2, 1, 1024, 2),
    "threshold_1025": lambda: grid_case("threshold_1025", 204, P2, 1, 1025, 2),
    "pairs": lambda: grid_case("pairs", 205, P2, 2, 515, 2),
    "dense": lambda: grid_case("dense", 206, P2, 2, 680, 16),
    "falloff": falloff_case,
    "l2p8_37": lambda: grid_case("l2p8_37", 208, [(8, 16), (4, 8)], 2, 37, 1, "slots"),
    "l2p8_515": lambda: grid_case("l2p8_515", 209, [(8, 16), (4, 8)], 2, 515, 2),
    "l1p16_37": lambda: grid_case("l1p16_37", 210, [(16, 16)], 2, 37, 1, "slots"),
    "l1p16_515": lambda: grid_case("l1p16_515", 211, [(16, 16)], 2, 515, 16),
    "one": one_case,
    "tiny": lambda: grid_case("tiny", 213, P2, 4, 7, 2),
}
BITS_CASES = {
    "bits_last_lds": lambda: grid_case("bits_last_lds", 214, BITS_LAST_LDS, 2, 515, 1, "slots"),
    "bits_memory": lambda: grid_case("bits_memory", 215, BITS_MEMORY, 2, 515, 1, "slots"),
}
ODD_SHAPES = {"odd_37": (ODD, 2, 37), "odd_111": (ODD, 3, 37), "odd_515": (ODD, 2, 515), "degenerate_37": (R.DEGENERATE_PYRAMID, 2, 37),
              "degenerate_515": (R.DEGENERATE_PYRAMID, 2, 515)}
ODD_FUSED_CASES = {n: functools.partial(odd_fused_case, n, 220 + i, *a) for i, (n, a) in enumerate(ODD_SHAPES.items())}
ODD_PLAIN_CASES = {n: functools.partial(R.random_case, 230 + i, a[1], a[0], Lq=a[2]) for i, (n, a) in enumerate(ODD_SHAPES.items())}


@functools.lru_cache(maxsize=None)
def case(name):
    """Built once, left unchanged."""
    return (EXACT_CASES.get(name) or BITS_CASES.get(name) or ODD_FUSED_CASES[name])()


# containment (slots_wave): NaN in level 0 at (y, x) = (1, 1) -- next to the (0, 0) that every invalid sample is clamped to --
# and inf in level 2 at (2, 5); one channel of one head each
POISON = ((0, 1 * 32 + 1, 2, 9, float("nan")), (1, 512 + 128 + 2 * 8 + 5, 5, 20, float("inf")))   # (image, token, head, channel, what)
