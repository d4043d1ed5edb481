"""GPU (-m gpu): the skinny linear layer's backward (csrc/linear.hip: egtr_linear_backward_acc_f32 / egtr_linear_backward_f32,
kernel linear_skinny_bwd_f32) and forward (egtr_linear_f32) called directly, against the float64 statement of
tests/skinny_backward_restated.py.

  * grid inputs (every sum exactly representable, whatever its order): ``torch.equal`` on every output of every case -- the M
    sweep through the weight-gradient tiles' load batches (M > 1024: second and later batches of a lane group's rows, the first
    runs of that loop trip under an assertion), both tile forms and their boundary, every count of reduction steps, every
    option of the entry (addends, aliased output, null outputs, alpha, ReLU mask);
  * outputs live NaN-filled inside larger NaN-filled allocations: nothing around them is written, everything in them is;
  * one inexact case (random normal inputs, alpha = 32^-0.5) against float64 within max(rounding bound, 4 x the float32 torch
    composition's own error);
  * containment of a NaN: exactly the row / column it belongs to;
  * refusals (status, nothing written); egtr_linear_backward_f32 = the bits of the acc entry without addends.
"""
import functools
import math

import pytest
import torch

import skinny_backward_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GUARD = 1024          # floats before and after an output (a multiple of 4: the output keeps its 16-byte alignment)


def _guarded(*shape):
    """A NaN-filled tensor of ``shape`` inside a larger NaN-filled allocation: (whole allocation, view)."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float32, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _untouched(whole, n):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + n:]).all())


def _status(entry, *args):
    from egtr_amd import _lib
    return getattr(_lib.lib(), entry)(_lib._stream(), *args)


def _run(c, dev_inp, entry="egtr_linear_backward_acc_f32", alpha=None):
    """The entry on the case: outputs in guarded NaN-filled buffers; returns {"gx", "gw", "gb"} (None where not asked for) after
    asserting that the guards are intact and that every output element is finite."""
    from egtr_amd import _lib
    g, y, x, w, a1, a2 = dev_inp
    M, K, N = c["M"], c["K"], c["N"]
    alpha = c["alpha"] if alpha is None else alpha
    bufs = {}
    if c["want_gx"]:
        bufs["gx"] = _guarded(M, K)
    if c["want_gw"]:
        bufs["gw"] = _guarded(N, K)
    if c["want_gb"]:
        bufs["gb"] = _guarded(N)
    p1 = a1 if c["add1"] else None
    p2 = a2 if c["add2"] else None
    if c["alias"] == "add1":       # the addend lives in the output buffer
        bufs["gx"][1].copy_(a1)
        p1 = bufs["gx"][1]
    if c["alias"] == "add2":
        bufs["gx"][1].copy_(a2)
        p2 = bufs["gx"][1]
    out = {k: bufs[k][1] if k in bufs else None for k in ("gx", "gw", "gb")}
    args = [g.data_ptr(), y.data_ptr() if c["relu"] else None, x.data_ptr(), w.data_ptr(), float(alpha), _lib.ptr(out["gx"]),
            _lib.ptr(out["gw"]), _lib.ptr(out["gb"]), M, K, N]
    if entry == "egtr_linear_backward_acc_f32":
        args += [_lib.ptr(p1), _lib.ptr(p2)]
    else:
        assert p1 is None and p2 is None
    _lib.launch(entry, *args)
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert _untouched(whole, view.numel()), (c["name"], k, "written outside the output")
        assert bool(torch.isfinite(view).all()), (c["name"], k, "an output element was not written")
    return out


@functools.lru_cache(maxsize=2)
def _dev_inputs(M, K, N):
    return tuple(t.to(DEV) for t in R.inputs(M, K, N))


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_grid_case_is_bit_exact(name):
    c = next(c for c in R.CASES if c["name"] == name)
    R.assert_exact(c, R.inputs(c["M"], c["K"], c["N"]))
    inp = _dev_inputs(c["M"], c["K"], c["N"])
    want = R.expected(c, inp)                      # float64 on the device: every sum is exact there too
    R.assert_float32_holds(want)
    got = _run(c, inp)
    for k in ("gx", "gw", "gb"):
        assert (got[k] is None) == (want[k] is None)
        if got[k] is not None:
            same = torch.equal(got[k], want[k].float())
            assert same, (name, k, int((got[k] != want[k].float()).sum()), float((got[k].double() - want[k]).abs().max()))


@pytest.mark.parametrize("M,K,N", [(33, 256, 256), (1025, 256, 256), (1025, 256, 1024)])
def test_plain_entry_gives_the_bits_of_the_acc_entry_without_addends(M, K, N):
    for relu in (True, False):
        c = R.case(M, K, N, relu=relu, alpha=0.25, tag="plain-entry")
        inp = _dev_inputs(M, K, N)
        a = _run(c, inp, entry="egtr_linear_backward_f32")
        b = _run(c, inp)
        want = R.expected(c, inp)
        for k in ("gx", "gw", "gb"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
            assert torch.equal(a[k], want[k].float()), k


def test_inexact_case_against_float64():
    """alpha = 32^-0.5 (as float32, which is what the entry receives), standard normal g, x, W and addends, (M, K, N) = (1025,
    256, 256), with the ReLU mask.  Bound per tensor: max(plain, 4 x the float32 torch composition's error), where plain is the
    rounding bound of a float32 sum of n products formed in blocks -- b terms per block, n / b blocks, any order inside: at most
    (b + n / b) u sum|terms|, least at b = sqrt(n) -- (2 sqrt(n) + 4) u max(sum of the |terms|) with u = 2^-24 (4: the products,
    alpha, two addends), taken over the tensor; a sum ordered worse than that is what it flags.  Measured on an MI355X
    (kernel / yardstick / plain): gx 1.87e-6 / 6.11e-6 / 5.7e-5, gw 3.82e-6 / 1.44e-5 / 2.9e-4, gb 2.15e-6 / 2.12e-6 / 3.3e-4."""
    M, K, N = R.INEXACT
    gen = torch.Generator().manual_seed(91)
    g, x, a1, a2 = (torch.randn(M, d, generator=gen).to(DEV) for d in (N, K, K, K))
    w = torch.randn(N, K, generator=gen).to(DEV)
    y = torch.relu(torch.randn(M, N, generator=gen)).to(DEV)
    alpha = float(torch.tensor(32 ** -0.5, dtype=torch.float32))
    c = R.case(M, K, N, relu=True, add1=True, add2=True, alpha=alpha, tag="inexact")
    inp = (g, y, x, w, a1, a2)
    want = R.expected(c, inp)
    got = _run(c, inp)
    # the float32 torch composition of the same statement
    gp = alpha * (g * (y > 0).float())
    yard = dict(gx=gp @ w + a1 + a2, gw=gp.t() @ x, gb=gp.sum(0))
    gpa = (alpha * g * (y > 0)).double().abs()
    u = 2.0 ** -24
    nx, nw = 2 * math.sqrt(N) + 4, 2 * math.sqrt(M) + 4
    plain = dict(gx=nx * u * float((gpa @ w.double().abs() + a1.double().abs() + a2.double().abs()).max()),
                 gw=nw * u * float((gpa.t() @ x.double().abs()).max()), gb=nw * u * float(gpa.sum(0).max()))
    for k in ("gx", "gw", "gb"):
        err = float((got[k].double() - want[k]).abs().max())
        yd = float((yard[k].double() - want[k]).abs().max())
        print(f"inexact {k}: kernel {err:.3e} yardstick {yd:.3e} ratio {err / max(yd, 1e-300):.2f} plain {plain[k]:.3e} "
              f"max|ref| {float(want[k].abs().max()):.2f}")
        assert yd > 0
        assert err <= max(plain[k], 4 * yd), (k, err, yd, plain[k])


def test_a_nan_stays_in_its_row_and_column():
    """(1057, 256, 256), 34 rows per lane group in batches of 32: rows 33 and 67 are the last of the two rows in the second
    batch of groups 0 and 1, rows 0 and 40 lie in first batches, row M - 1 is the row that out-of-range lanes re-read (30 of the
    32 slots of every second batch, and all but 3 slots of group 31, whose share is 3 rows). A NaN in g[m, n] (at an element the ReLU mask lets
    through) makes exactly gx[m, :], gw[n, :] and gb[n] non-finite; a NaN in x[M - 1, k] exactly gw[:, k]; everything else
    keeps the bits of the clean run."""
    M, K, N = R.CONTAINMENT
    c = R.case(M, K, N, relu=True, add1=True, tag="containment")
    g, y, x, w, a1, a2 = _dev_inputs(M, K, N)
    clean = _run_allowing_nan(c, (g, y, x, w, a1, a2))
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    assert -(-M // R.GROUPS) == 34 and R.BATCH == 32
    for m in (0, 33, 40, 67, M - 1):
        n = int(torch.nonzero(y[m] > 0)[3])
        gn = g.clone()
        gn[m, n] = NAN
        got = _run_allowing_nan(c, (gn, y, x, w, a1, a2))
        bad = {k: ~torch.isfinite(got[k]) for k in got}
        want_gx = torch.zeros(M, K, dtype=torch.bool, device=DEV)
        want_gx[m] = True
        want_gw = torch.zeros(N, K, dtype=torch.bool, device=DEV)
        want_gw[n] = True
        want_gb = torch.zeros(N, dtype=torch.bool, device=DEV)
        want_gb[n] = True
        for k, wb in (("gx", want_gx), ("gw", want_gw), ("gb", want_gb)):
            assert torch.equal(bad[k], wb), (m, n, k, int(bad[k].sum()), int(wb.sum()))
            assert torch.equal(got[k][~wb].view(torch.int32), clean[k][~wb].view(torch.int32)), (m, n, k)
    k0 = 77
    xn = x.clone()
    xn[M - 1, k0] = NAN
    got = _run_allowing_nan(c, (g, y, xn, w, a1, a2))
    wb = torch.zeros(N, K, dtype=torch.bool, device=DEV)
    wb[:, k0] = True
    assert torch.equal(~torch.isfinite(got["gw"]), wb)
    assert torch.equal(got["gw"][~wb].view(torch.int32), clean["gw"][~wb].view(torch.int32))
    for k in ("gx", "gb"):
        assert torch.equal(got[k].view(torch.int32), clean[k].view(torch.int32)), k


def _run_allowing_nan(c, inp):
    """_run without the all-finite assertion (the guards are still checked)."""
    from egtr_amd import _lib
    g, y, x, w, a1, a2 = inp
    M, K, N = c["M"], c["K"], c["N"]
    bufs = dict(gx=_guarded(M, K), gw=_guarded(N, K), gb=_guarded(N))
    _lib.launch("egtr_linear_backward_acc_f32", g.data_ptr(), y.data_ptr(), x.data_ptr(), w.data_ptr(), float(c["alpha"]),
                bufs["gx"][1].data_ptr(), bufs["gw"][1].data_ptr(), bufs["gb"][1].data_ptr(), M, K, N, a1.data_ptr(), None)
    torch.cuda.synchronize()
    for k, (whole, view) in bufs.items():
        assert _untouched(whole, view.numel()), (c["name"], k)
    return {k: v[1] for k, v in bufs.items()}


def test_refusals_launch_nothing():
    """N or K not a multiple of 64 and an addend 4 bytes off 16-byte alignment: EGTR_E_UNSUPPORTED (-3); an addend without
    grad_x: EGTR_E_ARG (-1).  The outputs keep their NaN fill."""
    M = 33

    def call(K, N, add1=None, gx=True):
        g = torch.ones(M, N, device=DEV)
        x = torch.ones(M, K, device=DEV)
        w = torch.ones(N, K, device=DEV)
        bx, bw, bb = _guarded(M, K), _guarded(N, K), _guarded(N)
        a = add1(M, K) if add1 is not None else None
        st = _status("egtr_linear_backward_acc_f32", g.data_ptr(), None, x.data_ptr(), w.data_ptr(), 1.0,
                     bx[1].data_ptr() if gx else None, bw[1].data_ptr(), bb[1].data_ptr(), M, K, N,
                     a.data_ptr() if a is not None else None, None)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b[0]).all()) for b in (bx, bw, bb)), "a refused call wrote something"
        return st

    def off_by_four_bytes(M, K):
        t = torch.zeros(M * K + 4, device=DEV)[1:1 + M * K].view(M, K)
        assert t.data_ptr() % 16 == 4
        return t

    assert call(256, 96) == -3 and call(256, 32) == -3
    assert call(96, 256) == -3 and call(32, 64) == -3
    assert call(256, 256, add1=off_by_four_bytes) == -3
    assert call(256, 256, add1=lambda M, K: torch.zeros(M, K, device=DEV), gx=False) == -1


@pytest.mark.parametrize("K", R.FORWARD_K)
def test_forward_entry_is_bit_exact_on_the_grids(K):
    """egtr_linear_f32 at one K per span instantiation (K / 16 = 4: generic, 16, 20: generic, 32, 64), N with partial column
    tiles, M with partial row tiles and more than one of them; bias, alpha and ReLU in the epilogue."""
    from egtr_amd import _lib
    for N in R.FORWARD_N:
        for M in R.FORWARD_M:
            x, w, b = R.forward_inputs(M, K, N)
            for alpha, relu, bias in ((0.25, True, True), (1.0, False, True), (0.25, False, False)):
                R.assert_exact_forward(x, w, b, alpha)
                xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
                want = R.expected_forward(xd, wd, bd if bias else torch.zeros_like(bd), alpha, relu)
                assert bool((want.float().double() == want).all())
                whole, yv = _guarded(M, N)
                _lib.launch("egtr_linear_f32", xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias else None, yv.data_ptr(), M,
                            K, N, float(alpha), 1 if relu else 0)
                torch.cuda.synchronize()
                assert _untouched(whole, M * N), (M, K, N)
                assert torch.equal(yv, want.float()), (M, K, N, alpha, relu, bias, int((yv != want.float()).sum()))
