"""GPU (-m gpu): the decoder self-attention core (csrc/self_attn.hip) at every register-tile slot, on shifted scores, and off its
shape range.  Inputs come from ``helpers.attn_grid_inputs`` / ``attn_shift`` / ``attn_dominant_keys`` (host checks of those:
tests/test_self_attention_inputs_cpu.py); the reference is the plain torch composition in fp64 on the device, the yardstick the
same composition in fp32.

The forward keeps NTW key tiles per wave (wave w owns tiles w, w + 4, ...; <NTW=4> for N <= 256, <NTW=10> up to 640).  What each
test resolves:
  * slot sweep (dominant keys): the key / value indexing of EVERY (wave, slot) of both instantiations, the ragged last tile, the
    -inf guard, the LDS merge (factors exactly 1 or 0), the (tile, head, batch) decode of the grid, the retained maps.  A
    mismatch at (b, h) names tile t = key // 16, i.e. wave t % 4, slot t // 4.  It does NOT see the accuracy of __expf, __logf or
    of the merge factors between 0 and 1: every probability is exactly 0 or 1.
  * shift invariance: the per-wave maximum, its cross-lane reduce and the cross-wave rescale exp(m_w - M) with scores near +-96
    (any missing maximum overflows or underflows); lse against fp64.  Bitwise equality under a shift says nothing about __expf's
    accuracy (the same arguments reach it at every shift): that is what the 2e-5 bound against fp64 at c = 0 is for.
  * backward / accumulate entry: both roles against fp64 autograd on plain, shifted and peaked rows; the p recomputed from a
    rounded lse is measured against the fp32 composition's own error.
  * containment, fall-offs: a NaN stays in its (b, row, h) slice; shapes the kernel does not serve take the announced torch
    composition (``ops._gate("self_attention")``) while the C entries keep refusing them.
Nothing here looks at the generated code."""
import functools
import math
import warnings

import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, N, M): every NTW=4 slot full / ragged tile 15 / first NTW=10 shape (wave 0 one tile ahead) / all 40 slots / ragged tile 39 /
# head counts other than 8
SHAPES = [(2, 256, 8), (2, 241, 8), (3, 257, 8), (5, 640, 8), (5, 625, 8), (3, 49, 5), (1, 33, 1)]
SHIFTS = (0.0, 96.0, -96.0)


def _id(s):
    return "B%d-N%d-M%d" % s


@functools.lru_cache(maxsize=None)
def _grid(B, N, M):
    """attn_grid_inputs on the device; shared between the tests and never written to."""
    return tuple(t.to(DEV) for t in Hh.attn_grid_inputs(2000 + 7 * N + M, B, N, M))


@functools.lru_cache(maxsize=None)
def _plain(B, N, M, peak=1.0):
    g = torch.Generator().manual_seed(50 + N + M)
    q, k, v, go = (torch.randn(B, N, M * 32, generator=g) for _ in range(4))
    return tuple(t.to(DEV) for t in (q * 32 ** -0.5 * peak, k, v, go))


def _forward(q, k, v, M, want_lse=False):
    """The C entry for the operands' dtype, called directly; every output is NaN-filled first, so a row the kernel never writes
    shows.  Returns (out, q_heads, k_heads, lse)."""
    from egtr_amd import _lib
    B, N, MD = q.shape
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    out = torch.full_like(q, float("nan"))
    qh = torch.full((B, M, N, MD // M), float("nan"), dtype=q.dtype, device=q.device)
    kh = torch.full_like(qh, float("nan"))
    lse = None
    if q.dtype == torch.float32:
        lse = torch.full((B, M, N), float("nan"), device=q.device) if want_lse else None
        _lib.launch("egtr_self_attn_forward_f32", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, N, M, MD // M, out.data_ptr(),
                    qh.data_ptr(), kh.data_ptr(), _lib.ptr(lse))
    else:
        assert q.dtype == torch.bfloat16 and not want_lse
        _lib.launch("egtr_self_attn_forward_bf16", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, N, M, MD // M, out.data_ptr(),
                    qh.data_ptr(), kh.data_ptr())
    return out, qh, kh, lse


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _biteq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ulp(x):
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def _plain_bound(g):
    return 5e-5 * max(1.0, float(g.abs().max()))


def _err(a, ref):
    return float((a.double() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ 1. slot sweep
def _check_dominant(out, v, keys, M):
    bad = Hh.attn_dominant_mismatches(out, v, keys, M)
    assert not bad, "out[b, :, h] != v[b, key, h] at (b, h, tile -> wave, slot): " + ", ".join(
        f"({b}, {h}, {t} -> {t % 4}, {t // 4})" for b, h, t in bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,M", SHAPES, ids=[_id(s) for s in SHAPES])
def test_slot_sweep_a_dominant_key_in_every_tile_returns_its_value_row_bitwise(B, N, M, dtype):
    """One key per (b, h) scores >= 104 above the rest: every other probability is exactly 0, exp(0) = 1, tot = 1, the merge
    factors are 1 or 0, so out[b, :, h] is v[b, key, h] bit for bit in all N rows (bf16: of the bf16-rounded v).  B * M >= ntile
    makes every tile dominant for some (b, h); (1, 33, 1) has one (b, h) for three tiles and walks them by rotation instead."""
    q, k, v, _ = _grid(B, N, M)
    ntile = (N + 15) // 16
    assert B * M >= ntile or (B, N, M) == (1, 33, 1)
    tiles = set()
    for rot in ([0] if B * M >= ntile else range(ntile)):
        kd, keys = Hh.attn_dominant_keys(k.cpu(), B, N, M, rot=rot)
        tiles |= set((keys // 16).flatten().tolist())
        qd, kd, vd = q.to(dtype), kd.to(DEV).to(dtype), v.to(dtype)
        out, qh, kh, _ = _forward(qd, kd, vd, M)
        _check_dominant(out, vd, keys, M)
        assert _biteq(qh, Hh.attn_heads(qd, M).contiguous()) and _biteq(kh, Hh.attn_heads(kd, M).contiguous())
    assert tiles == set(range(ntile))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_slot_sweep_assertion_catches_a_dropped_tile_and_a_missing_maximum(dtype):
    """Teeth of the test above, without touching the library: the same assertion on two deliberately wrong torch compositions at
    (2, 256, 8) -- one that never sees tile 15 (wave 3, slot 3: the slot no earlier test filled), one that skips the maximum."""
    B, N, M = 2, 256, 8
    q, k, v, _ = _grid(B, N, M)
    kd, keys = Hh.attn_dominant_keys(k.cpu(), B, N, M)
    kd, vd = kd.to(DEV), v.to(dtype)
    assert 15 in (keys // 16).flatten().tolist()
    _check_dominant(Hh.attn_compose(q, kd, vd.float(), M).to(dtype), vd, keys, M)            # the intact composition passes
    with pytest.raises(AssertionError, match=r"15 -> 3, 3"):
        _check_dominant(Hh.attn_compose(q, kd, vd.float(), M, drop_tile=15).to(dtype), vd, keys, M)
    with pytest.raises(AssertionError):
        _check_dominant(Hh.attn_compose(q, kd, vd.float(), M, skip_max=True).to(dtype), vd, keys, M)


# ------------------------------------------------------------------------------------------------ 2. shift invariance
def _check_shift_invariant(fn, q, k, v, M, ref64=None):
    """``fn(q, k, v) -> out``: finite and bitwise the same at c = 0, 96, -96; within 2e-5 of fp64 at c = 0 when ``ref64`` is
    given.  Returns the c = 0 output."""
    outs = [fn(q, Hh.attn_shift(k, M, c), v) for c in SHIFTS]
    for c, o in zip(SHIFTS, outs):
        assert bool(torch.isfinite(o).all()), f"non-finite output at shift {c}"
        assert _biteq(o, outs[0]), f"output at shift {c} differs from shift 0"
    if ref64 is not None:
        e = _err(outs[0], ref64)
        print(f"forward |out - fp64| = {e:.3e}")
        assert e < 2e-5
    return outs[0]


@pytest.mark.parametrize("B,N,M", SHAPES, ids=[_id(s) for s in SHAPES])
def test_forward_is_bitwise_shift_invariant_and_lse_follows_the_shift(B, N, M):
    """Grid inputs: s and s - max are exact fp32 numbers at every shift, so the kernel's probabilities and hence its output are
    the same bits for c = 0, 96, -96 (fp32 and bf16); a missing or partial maximum gives inf / NaN at +96 and 0 / 0 at -96.
    out at c = 0 meets the suite's 2e-5 against fp64.

    lse (``mall + __logf(tot)``: two roundings) against fp64 logsumexp of the exact scores, bound max(4 x the error of fp32
    torch.logsumexp on the same scores, 4 ulp of the largest |lse|).  Measured on an MI355X, the largest over these seven shapes:
    kernel error 1.00e-6 at c = 0 (|lse| <= 11.3) and 4.28e-6 at c = +-96 (|lse| <= 107.3: half an ulp there is 3.8e-6);
    yardstick 1.01e-6 and 4.26e-6, per shape within 15 % of the kernel's error either way; bound 3.8e-6 .. 4.0e-6 and 3.05e-5 (the
    4 ulp term decides at c = +-96).  out against fp64 at c = 0: at most 2.6e-6."""
    q, k, v, _ = _grid(B, N, M)
    ref = Hh.attn_compose(q.double(), k.double(), v.double(), M)
    _check_shift_invariant(lambda a, b, c: _forward(a, b, c, M)[0], q, k, v, M, ref64=ref)
    _check_shift_invariant(lambda a, b, c: _forward(a.bfloat16(), b.bfloat16(), c.bfloat16(), M)[0], q, k, v, M)
    s64 = Hh.attn_scores(q.double(), k.double(), M)
    for c in SHIFTS:
        lse = _forward(q, Hh.attn_shift(k, M, c), v, M, want_lse=True)[3]
        want = torch.logsumexp(s64 + c, -1)
        yard = _err(torch.logsumexp((s64 + c).float(), -1), want)
        err, bound = _err(lse, want), max(4 * yard, 4 * _ulp(float(want.abs().max())))
        print(f"lse shift {c:+.0f}: kernel {err:.3e} yardstick {yard:.3e} bound {bound:.3e} max|lse| {float(want.abs().max()):.2f}")
        assert yard > 0 and err <= bound


def test_shift_assertions_catch_a_missing_maximum_and_a_dropped_tile():
    """Teeth: the composition without the maximum fails the bitwise shift check (inf / inf at +96); the one that never sees tile
    15 is shift-invariant by construction and is caught by the 2e-5 bound against fp64 instead."""
    B, N, M = 2, 256, 8
    q, k, v, _ = _grid(B, N, M)
    ref = Hh.attn_compose(q.double(), k.double(), v.double(), M)
    _check_shift_invariant(lambda a, b, c: Hh.attn_compose(a, b, c, M), q, k, v, M, ref64=ref)   # the intact composition passes
    with pytest.raises(AssertionError, match="shift 96"):
        _check_shift_invariant(lambda a, b, c: Hh.attn_compose(a, b, c, M, skip_max=True), q, k, v, M, ref64=ref)
    with pytest.raises(AssertionError):
        _check_shift_invariant(lambda a, b, c: Hh.attn_compose(a, b, c, M, drop_tile=15), q, k, v, M, ref64=ref)


# ------------------------------------------------------------------------------------------------ 3. backward
def _autograd(fn, q, k, v, go):
    """Gradients of sum(out * go) (+ a second scalar when ``fn`` returns a pair) with respect to q, k, v."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    res = fn(q, k, v)
    out, extra = res if isinstance(res, tuple) else (res, 0.0)
    ((out * go).sum() + extra).backward()
    return q.grad, k.grad, v.grad


def _kernel_grads(q, k, v, go, M):
    from egtr_amd.ops import DecoderSelfAttentionFunction
    return _autograd(lambda a, b, c: DecoderSelfAttentionFunction.apply(a, b, c, M, False)[0], q, k, v, go)


def _bwd_inputs(kind, B, N, M):
    if kind == "shift96":
        q, k, v, go = _grid(B, N, M)
        return q, Hh.attn_shift(k, M, 96.0), v, go
    return _plain(B, N, M, 8.0 if kind == "peaked" else 1.0)


@pytest.mark.parametrize("kind", ["plain", "shift96", "peaked"])
@pytest.mark.parametrize("B,N,M", SHAPES, ids=[_id(s) for s in SHAPES])
def test_backward_against_fp64_autograd(B, N, M, kind):
    """egtr_self_attn_backward_f32 through DecoderSelfAttentionFunction against fp64 autograd of the torch composition.
    plain (standard normal, q * 32^-0.5): the suite's bound 5e-5 * max(1, |g|max).  shift96 (grid inputs, every score + 96) and
    peaked (plain q * 8): the fp32 torch composition itself leaves that bound (a score gradient that sums to zero is multiplied
    by k's component 0 = 96; rows with one probability near 1), so the bound is max(plain, 4 x the fp32 composition's own error
    against fp64, on the device) per gradient -- 4 for the kernel's p recomputed from a rounded lse where torch keeps p.
    Measured on an MI355X, the largest over the seven shapes of kernel error / yardstick (and of kernel error / bound):
        plain    grad_q 2.09 (0.018)   grad_k 1.90 (0.019)   grad_v  1.88 (0.018)
        shift96  grad_q 1.88 (0.47)    grad_k 8.70 (0.055)   grad_v 27.8  (0.059)
        peaked   grad_q 1.78 (0.088)   grad_k 1.60 (0.076)   grad_v  1.62 (0.027)
    The large shift96 ratios are the rounded lse at work: |lse| ~ 107 carries an absolute error of up to 4e-6, which the kernel's
    p = exp(s - lse) turns into that RELATIVE error of every probability (grad_v 9.9e-6, grad_k 2.2e-5 at most, both well inside the
    plain bound that decides there); torch keeps its p.  grad_q at shift96 is the one case the 4 x yardstick term decides: kernel
    6.8e-4 at most against a yardstick of 3.6e-4 at (5, 640, 8), where the plain bound is 2.9e-4."""
    q, k, v, go = _bwd_inputs(kind, B, N, M)
    got = _kernel_grads(q, k, v, go, M)
    ref = _autograd(lambda a, b, c: Hh.attn_compose(a, b, c, M), q.double(), k.double(), v.double(), go.double())
    y32 = _autograd(lambda a, b, c: Hh.attn_compose(a, b, c, M), q, k, v, go)
    for name, g, r, y in zip(("grad_q", "grad_k", "grad_v"), got, ref, y32):
        err, yard, plain = _err(g, r), _err(y, r), _plain_bound(r)
        print(f"bwd {kind} {name}: kernel {err:.3e} yardstick {yard:.3e} ratio {err / max(yard, 1e-300):.2f} plain {plain:.3e} "
              f"|g|max {float(r.abs().max()):.2f}")
        assert yard > 0
        assert err <= (plain if kind == "plain" else max(plain, 4 * yard)), (name, err, yard, plain)


@pytest.mark.parametrize("B,N,M", SHAPES, ids=[_id(s) for s in SHAPES])
def test_backward_under_dominant_keys_routes_the_whole_gradient_to_one_value_row(B, N, M):
    """Every query row of (b, h) attends to one key with probability exactly 1 (lse is that key's score exactly, exp(0) = 1,
    exp(< -104) = 0): grad_v[b, key, h] is the column sum of the upstream gradient and every other grad_v row is exactly 0."""
    q, k, v, go = _grid(B, N, M)
    kd, keys = Hh.attn_dominant_keys(k.cpu(), B, N, M)
    gv = _kernel_grads(q, kd.to(DEV), v, go, M)[2]
    want = Hh.attn_heads(go.double(), M).sum(2)                                          # [B, M, D]
    gvh = Hh.attn_heads(gv, M)
    sel = torch.zeros(B, M, N, dtype=torch.bool, device=DEV)
    sel.scatter_(2, keys.to(DEV)[..., None], True)
    assert _err(gvh[sel].view(B, M, 32), want) <= _plain_bound(want)
    assert bool((gvh[~sel] == 0).all())


# ------------------------------------------------------------------------------------------------ 4. accumulate entry
def _launch_bwd(entry, q, k, v, out, lse, go, M, *adds):
    from egtr_amd import _lib
    B, N, MD = q.shape
    g = [torch.full_like(q, float("nan")) for _ in range(3)]
    _lib.launch(entry, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), go.data_ptr(), B, N, M, MD // M,
                g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), *[_lib.ptr(a) for a in adds])
    return g


@pytest.mark.parametrize("B,N,M", [(2, 257, 8), (3, 49, 5)], ids=["B2-N257-M8", "B3-N49-M5"])
def test_accumulate_backward_entry_against_fp64(B, N, M):
    """egtr_self_attn_backward_acc_f32 called directly (the backward of the fused decoder training node): grad_q / grad_k are the
    fp64 gradient plus the addend within the plain bound, grad_v does not change, null addends give the bits of
    egtr_self_attn_backward_f32, and an addend that is not 16-byte aligned is refused before anything is launched."""
    from egtr_amd import _lib
    q, k, v, go = _plain(B, N, M)
    out, _, _, lse = _forward(q, k, v, M, want_lse=True)
    g = torch.Generator().manual_seed(N)
    add_q, add_k = (torch.randn(B, N, M * 32, generator=g).to(DEV) for _ in range(2))
    acc = _launch_bwd("egtr_self_attn_backward_acc_f32", q, k, v, out, lse, go, M, add_q, add_k)
    nul = _launch_bwd("egtr_self_attn_backward_acc_f32", q, k, v, out, lse, go, M, None, None)
    old = _launch_bwd("egtr_self_attn_backward_f32", q, k, v, out, lse, go, M)
    ref = _autograd(lambda a, b, c: Hh.attn_compose(a, b, c, M), q.double(), k.double(), v.double(), go.double())
    for a, b in zip(nul, old):
        assert bool(torch.isfinite(a).all()) and _biteq(a, b)
    assert _biteq(acc[2], nul[2])
    for name, got, r, add in (("grad_q", acc[0], ref[0], add_q), ("grad_k", acc[1], ref[1], add_k), ("grad_v", acc[2], ref[2], None)):
        want = r if add is None else r + add.double()
        print(f"acc {name}: {_err(got, want):.3e} plain {_plain_bound(r):.3e}")
        assert _err(got, want) <= _plain_bound(r)
    # one addend at a time: each lands on its own gradient only
    only_q = _launch_bwd("egtr_self_attn_backward_acc_f32", q, k, v, out, lse, go, M, add_q, None)
    assert _biteq(only_q[0], acc[0]) and _biteq(only_q[1], nul[1]) and _biteq(only_q[2], nul[2])
    flat = torch.randn(B * N * M * 32 + 1, generator=g).to(DEV)
    off = flat[1:].view(B, N, M * 32)
    assert off.data_ptr() % 16 == 4
    for adds in ((off, None), (None, off), (off, add_k)):
        with pytest.raises(_lib.EgtrHipError, match="status -3"):
            _launch_bwd("egtr_self_attn_backward_acc_f32", q, k, v, out, lse, go, M, *adds)


# ------------------------------------------------------------------------------------------------ 5. containment
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_nan_query_row_stays_in_its_own_slice(dtype):
    """A NaN in one q row of one head makes exactly that (b, row, h) slice of out non-finite; everything else keeps the bits of
    the clean run (the query is a column of the score MFMA, the row statistics stay in the lanes of that column)."""
    B, N, M = 2, 49, 8
    q, k, v, _ = (t.to(dtype) for t in _plain(B, N, M))
    clean = _forward(q, k, v, M)[0]
    assert bool(torch.isfinite(clean).all())
    for b, row, h in ((1, 37, 5), (0, 48, 0), (0, 0, 7)):
        qn = q.clone()
        qn[b, row, h * 32 + 3] = float("nan")
        out = _forward(qn, k, v, M)[0]
        hit = torch.zeros(B, N, M * 32, dtype=torch.bool, device=DEV)
        hit[b, row, h * 32:(h + 1) * 32] = True
        assert not bool(torch.isfinite(out[hit]).any())
        assert torch.equal(_bits(out)[~hit], _bits(clean)[~hit])


# ------------------------------------------------------------------------------------------------ 6. fall-offs
@pytest.fixture
def fallbacks(monkeypatch):
    from egtr_amd import ops
    monkeypatch.setattr(ops, "FALLBACKS", {})
    monkeypatch.setattr(ops, "STRICT_FAST_PATH", False)
    return ops


OFF_PATH = [(1, 641, 256), (1, 700, 256), (2, 50, 512)]


@pytest.mark.parametrize("B,N,MD", OFF_PATH, ids=["N641", "N700", "head_dim64"])
def test_unserved_shapes_take_the_announced_torch_composition(fallbacks, B, N, MD):
    """More than 640 queries, or head_dim 64: ``ops.decoder_self_attention`` leaves the kernel through the "self_attention" gate
    (counted, announced once, an error under STRICT_FAST_PATH) and computes the plain composition: forward within 2e-5 of fp64,
    gradients -- through the output AND through the [B, M, N, D] maps -- within 5e-5 * max(1, |g|max)."""
    ops, M = fallbacks, 8
    g = torch.Generator().manual_seed(N + MD)
    q, k, v, go = (torch.randn(B, N, MD, generator=g).to(DEV) for _ in range(4))
    q = q * (MD // M) ** -0.5
    gqh, gkh = (torch.randn(B, M, N, MD // M, generator=g).to(DEV) for _ in range(2))

    def product(a, b, c):
        o, qh, kh = ops.decoder_self_attention(a, b, c, M, want_maps=True)
        assert qh.shape == kh.shape == (B, M, N, MD // M)
        assert torch.equal(qh, Hh.attn_heads(a, M)) and torch.equal(kh, Hh.attn_heads(b, M))
        return o, (qh * gqh).sum() + (kh * gkh).sum()

    def ref_fn(a, b, c):
        return Hh.attn_compose(a, b, c, M), (Hh.attn_heads(a, M) * gqh).sum() + (Hh.attn_heads(b, M) * gkh).sum()

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            out, qh, kh = ops.decoder_self_attention(q, k, v, M, want_maps=True)
            out2, none_q, none_k = ops.decoder_self_attention(q, k, v, M, want_maps=False)
    assert ops.FALLBACKS == {"self_attention": 2}
    assert len([x for x in w if "self_attention" in str(x.message)]) == 1
    assert none_q is None and none_k is None and torch.equal(out, out2)
    ref = Hh.attn_compose(q.double(), k.double(), v.double(), M)
    assert _err(out, ref) < 2e-5
    got = _autograd(product, q, k, v, go)
    want = _autograd(ref_fn, q.double(), k.double(), v.double(), go.double())
    for a, r in zip(got, want):
        assert _err(a, r) <= _plain_bound(r)
    # bf16 operands: the same route in bf16 (the bf16 entry refuses these shapes as well).  A routing check: dtype, layout, and
    # the value of the same bf16 composition evaluated again (within two bf16 steps of the largest output, should the vendor
    # library pick another GEMM solution the second time)
    b16 = [t.bfloat16() for t in (q, k, v)]
    ob, qb, kb = ops.decoder_self_attention(*b16, M, want_maps=True)
    assert ob.dtype == qb.dtype == kb.dtype == torch.bfloat16 and ob.shape == out.shape and ops.FALLBACKS["self_attention"] == 4
    assert torch.equal(qb, Hh.attn_heads(b16[0], M)) and torch.equal(kb, Hh.attn_heads(b16[1], M))
    again = Hh.attn_compose(*b16, M)
    assert _err(ob, again.double()) <= 2.0 ** -7 * float(again.abs().max())
    fallbacks.STRICT_FAST_PATH = True
    with pytest.raises(ops.FastPathError, match="self_attention"):
        ops.decoder_self_attention(q, k, v, M)


def test_the_largest_served_shape_is_not_a_fall_off(fallbacks):
    ops = fallbacks
    fallbacks.STRICT_FAST_PATH = True
    q, k, v, go = _plain(1, 640, 8)
    out = ops.decoder_self_attention(q, k, v, 8, want_maps=False)[0]
    ob = ops.decoder_self_attention(q.bfloat16(), k.bfloat16(), v.bfloat16(), 8, want_maps=False)[0]
    assert ops.FALLBACKS == {}
    assert _biteq(out, _forward(q, k, v, 8)[0]) and _biteq(ob, _forward(q.bfloat16(), k.bfloat16(), v.bfloat16(), 8)[0])
    got = _kernel_grads(q, k, v, go, 8)
    via_ops = _autograd(lambda a, b, c: ops.decoder_self_attention(a, b, c, 8, want_maps=False)[0], q, k, v, go)
    assert all(_biteq(a, b) for a, b in zip(got, via_ops)) and ops.FALLBACKS == {}


def test_a_512_wide_attention_module_runs_and_equals_its_explicit_route(fallbacks):
    """DeformableDetrMultiheadAttention(512, 8) (head_dim 64) and a 700-query call of the 256-wide module on the device: the
    fused route (now the announced composition) equals the module's own ``_attention_with_map`` route."""
    from egtr_amd.deformable_detr import DeformableDetrMultiheadAttention
    ops = fallbacks
    for width, n in ((512, 50), (256, 700)):
        torch.manual_seed(width)
        m = DeformableDetrMultiheadAttention(width, 8).to(DEV).eval()
        x, pos = torch.randn(2, n, width, device=DEV), torch.randn(2, n, width, device=DEV)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.no_grad():
                o, w_none, qm, km = m(x, position_embeddings=pos, output_attention_states=True)
                o_map, w_map, _, _ = m(x, position_embeddings=pos, output_attentions=True)
        assert w_none is None and w_map.shape == (2, 8, n, n) and qm.shape == km.shape == (2, 8, n, width // 8)
        assert bool(torch.isfinite(o).all()) and float((o - o_map).abs().max()) < 2e-5
    assert ops.FALLBACKS == {"self_attention": 2}


def test_the_c_entries_still_refuse_what_they_do_not_serve():
    from egtr_amd import _lib
    h = _lib.lib()
    for B, N, M, D in ((1, 641, 8, 32), (1, 50, 8, 64)):
        q = torch.zeros(B, N, M * D, device=DEV)
        out = torch.zeros_like(q)
        st = h.egtr_self_attn_forward_f32(_lib._stream(), q.data_ptr(), q.data_ptr(), q.data_ptr(), B, N, M, D, out.data_ptr(),
                                          None, None, None)
        assert st == -3 and b"not supported" in h.egtr_status_string(st)
        qb, ob = q.bfloat16(), out.bfloat16()
        assert h.egtr_self_attn_forward_bf16(_lib._stream(), qb.data_ptr(), qb.data_ptr(), qb.data_ptr(), B, N, M, D,
                                             ob.data_ptr(), None, None) == -3
    with pytest.raises(_lib.EgtrHipError):
        _forward(torch.zeros(1, 641, 256, device=DEV), torch.zeros(1, 641, 256, device=DEV),
                 torch.zeros(1, 641, 256, device=DEV), 8)
