"""GPU (-m gpu): dropout + residual + LayerNorm forward / backward (csrc/enc_train.hip: dropout_add_layernorm_256, _bwd,
partial_final_f32; ops.dropout_add_layernorm / ops.dropout_add_layernorm_backward) at the row counts where their launches
change shape: a single row, a partial last workgroup (4 rows per workgroup: 1, 3, 5, 37), and the switch from one row per wave
to eight at 16384 rows (16383, 16384, 16385, 16384 + 37: partial waves and a partial last workgroup of 32 rows).

Reference: float64 autograd of layer_norm(res + keep * scale * x); yardstick: the same composition in float32.  Every quantity
is held to max(plain bound, 4 x the yardstick's error) -- y, grad_sum and grad_x row by row, d gamma / d beta / d bias against the
float64 column sums.  The plain bounds (u = 2^-24):

  * rows: the statistics are sums of 256 terms; summed pairwise (depth 8) each carries at most 8 u sum|terms|.  y chains the
    mean, the variance, rsqrt and the affine map: 32 u (max|gamma| max|xhat| + max|y|) per row.  grad_sum = rstd (a - mean(a) -
    xhat mean(a xhat)) adds two more such sums on top of the forward's: 64 u rstd (max|a| + |mean(a)| + max|xhat| |mean(a xhat)|),
    a = grad_y gamma; grad_x is grad_sum times keep * scale.
  * column sums over n rows: formed in blocks (b terms per block, n / b blocks, any order inside) a sum carries at most
    (b + n / b) u sum|terms|, least at b = sqrt(n): (2 sqrt(n) + 32) u max over the columns of sum|terms| (32 for the error the
    terms themselves carry).  One lost row of O(1) terms is far outside it at every row count here.

Outputs are written into NaN-filled buffers with NaN guard rows behind them.  The clamp branch (the encoder node's "clamped
elements pass no gradient") is checked against a float64 statement of exactly that rule.

Measured on an MI355X, the largest kernel error / yardstick over the row counts: y 1.14, grad_sum 1.81 (one row), grad_x 1.00,
d gamma 4.10 and d beta 2.82 (16383 rows: 1.94e-4 and 1.32e-4 against yardsticks of 4.73e-5 and 4.69e-5, on sums of magnitude
395 and 336; the plain bounds, 0.18 and 0.23, decide there), d bias 1.61; error / bound at most 0.06.  Clamp branch: ratios 0.50 .. 1.16."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
P_DROP, SCALE, EPS = 0.25, 4.0 / 3.0, 1e-5
ROWS = (1, 3, 4, 5, 37, 16383, 16384, 16385, 16384 + 37)
GUARD_ROWS = 8


def _inputs(rows, seed=0):
    g = torch.Generator().manual_seed(1000 + rows + seed)
    x, r, gy = (torch.randn(rows, 256, generator=g).to(DEV) for _ in range(3))
    keep = (torch.rand(rows, 256, generator=g) < 1.0 - P_DROP).to(torch.uint8).to(DEV)
    w = (torch.rand(256, generator=g) + 0.5).to(DEV)
    b = torch.randn(256, generator=g).to(DEV)
    return x, r, gy, keep, w, b


def _guarded(rows):
    whole = torch.full((rows + GUARD_ROWS, 256), NAN, dtype=torch.float32, device=DEV)
    return whole, whole[:rows]


def _forward(x, r, keep, scale, w, b, flag=None):
    from egtr_amd import _lib
    rows = x.shape[0]
    whole, y = _guarded(rows)
    _lib.launch("egtr_dropout_add_layernorm_f32", x.data_ptr(), r.data_ptr(), _lib.ptr(keep), float(scale), w.data_ptr(),
                b.data_ptr(), y.data_ptr(), rows, 256, EPS, _lib.ptr(flag))
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole[rows:]).all()), "y: written behind the last row"
    return y


def _backward(x, r, keep, scale, w, gy, flag=None, y_out=None, clamp_value=0.0):
    """The backward entry with guarded outputs: (grad_sum, grad_x or None, [d gamma | d beta | d bias])."""
    from egtr_amd import _lib
    rows = x.shape[0]
    wgs, gs = _guarded(rows)
    wgx, gx = _guarded(rows) if keep is not None else (None, None)
    ws = torch.full((int(_lib.lib().egtr_dropout_add_layernorm_backward_workspace_floats(rows)),), NAN, device=DEV)
    out = torch.full((768 + 256,), NAN, device=DEV)
    _lib.launch("egtr_dropout_add_layernorm_backward_f32", x.data_ptr(), r.data_ptr(), _lib.ptr(keep), float(scale),
                w.data_ptr(), gy.data_ptr(), _lib.ptr(flag), _lib.ptr(y_out), float(clamp_value), gs.data_ptr(), _lib.ptr(gx),
                ws.data_ptr(), out.data_ptr(), rows, 256, EPS)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wgs[rows:]).all()), "grad_sum: written behind the last row"
    assert wgx is None or bool(torch.isnan(wgx[rows:]).all()), "grad_x: written behind the last row"
    assert bool(torch.isnan(out[768:]).all())
    return gs, gx, out[:768]


def _compose(x, r, gy, keep, w, b, dtype):
    """layer_norm(res + keep * scale * x) under autograd in ``dtype`` (no keep mask: no scale either, as the kernel has it): y,
    d res, d x, d gamma, d beta, d bias."""
    x_, r_, w_, b_ = (t.detach().to(dtype).requires_grad_(True) for t in (x, r, w, b))
    d = x_ * keep.to(dtype) * SCALE if keep is not None else x_
    y = F.layer_norm(r_ + d, (256,), w_, b_, EPS)
    y.backward(gy.to(dtype))
    return dict(y=y.detach(), gs=r_.grad, gx=x_.grad, dgamma=w_.grad, dbeta=b_.grad, dbias=x_.grad.sum(0))


def _row_scales(x, r, gy, keep, w):
    """Per row, in float64: the magnitudes the plain bounds of y and grad_sum are stated in."""
    v = r.double() + (x.double() * keep.double() * SCALE if keep is not None else x.double())
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + EPS)
    h = (v - mean) * rstd
    a = gy.double() * w.double()
    hmax, amax = h.abs().max(1).values, a.abs().max(1).values
    s_gs = rstd[:, 0] * (amax + a.mean(1).abs() + hmax * (a * h).mean(1).abs())
    return float(w.abs().max()) * hmax, s_gs, h


def _check_rows(name, got, want, yard, plain):
    err = (got.double() - want).abs().max(1).values
    yd = (yard.double() - want).abs().max(1).values
    bound = torch.maximum(plain, 4 * yd)
    worst = int((err / bound).argmax())
    print(f"{name}: kernel {float(err.max()):.3e} yardstick {float(yd.max()):.3e} ratio {float(err.max() / yd.max()):.2f} "
          f"plain {float(plain.max()):.3e}; worst row {worst}: {float(err[worst]):.3e} of {float(bound[worst]):.3e}")
    assert float(yd.max()) > 0
    assert bool((err <= bound).all()), (name, worst, float(err[worst]), float(bound[worst]))


def _check_sums(name, got, want, yard, plain):
    err, yd = float((got.double() - want).abs().max()), float((yard.double() - want).abs().max())
    print(f"{name}: kernel {err:.3e} yardstick {yd:.3e} ratio {err / max(yd, 1e-300):.2f} plain {plain:.3e} "
          f"max|ref| {float(want.abs().max()):.3f}")
    assert yd > 0
    assert err <= max(plain, 4 * yd), (name, err, yd, plain)


@pytest.mark.parametrize("with_keep", [True, False])
@pytest.mark.parametrize("rows", ROWS)
def test_row_edges_against_float64(rows, with_keep):
    from egtr_amd import ops
    x, r, gy, keep, w, b = _inputs(rows)
    keep = keep if with_keep else None
    scale = SCALE if with_keep else 1.0
    ref = _compose(x, r, gy, keep, w, b, torch.float64)
    yard = _compose(x, r, gy, keep, w, b, torch.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = _forward(x, r, keep, scale, w, b, flag=flag)
    gs, gx, gbb = _backward(x, r, keep, scale, w, gy)
    assert int(flag) == 0
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gbb).all())
    s_y, s_gs, h = _row_scales(x, r, gy, keep, w)
    tag = f"rows {rows} {'keep' if with_keep else 'no keep'}"
    _check_rows(f"{tag} y", y, ref["y"], yard["y"], 32 * U * (s_y + ref["y"].abs().max(1).values))
    _check_rows(f"{tag} grad_sum", gs, ref["gs"], yard["gs"], 64 * U * s_gs)
    if with_keep:
        assert bool(torch.isfinite(gx).all())
        _check_rows(f"{tag} grad_x", gx, ref["gx"], yard["gx"], 64 * U * s_gs * scale)
        assert bool((gx[keep == 0] == 0).all())
    else:
        assert gx is None
    n = 2 * math.sqrt(rows) + 32
    g64 = gy.double()
    _check_sums(f"{tag} d gamma", gbb[:256], ref["dgamma"], yard["dgamma"], n * U * float((g64 * h).abs().sum(0).max()))
    if rows == 1:   # a sum of ONE float32 term has no rounding: the yardstick's error is exactly 0 and so must the kernel's be
        assert float((yard["dbeta"].double() - ref["dbeta"]).abs().max()) == 0
        print(f"{tag} d beta: one term, compared bit for bit")
        assert torch.equal(gbb[256:512], gy[0])
    else:
        _check_sums(f"{tag} d beta", gbb[256:512], ref["dbeta"], yard["dbeta"], n * U * float(g64.abs().sum(0).max()))
    _check_sums(f"{tag} d bias", gbb[512:], ref["dbias"], yard["dbias"], n * U * float(ref["gx"].abs().sum(0).max()))
    # the package's wrappers are these launches
    y2 = ops.dropout_add_layernorm(x, r, keep, scale, w, b, EPS)
    gs2, gx2, gbb2 = ops.dropout_add_layernorm_backward(x, r, keep, scale, w, EPS, gy)
    assert torch.equal(y2, y) and torch.equal(gs2, gs) and torch.equal(gbb2, gbb)
    assert torch.equal(gx2, gx) if with_keep else gx2 is gs2


# ---------------------------------------------------------------------------------------------------------------- clamp branch
def _rule(x, r, gy, keep, w, y_out, cv, dtype):
    """The backward with the clamp rule, written out: elements with |y_out| >= cv or a NaN y_out pass no gradient."""
    x, r, gy, w = (t.to(dtype) for t in (x, r, gy, w))
    v = r + x * keep.to(dtype) * SCALE
    mean = v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + EPS)
    h = (v - mean) * rstd
    gm = torch.where(y_out.to(dtype).abs() < cv, gy, torch.zeros_like(gy))        # (a NaN compares false)
    a = gm * w
    s = rstd * (a - a.mean(1, keepdim=True) - h * (a * h).mean(1, keepdim=True))
    return dict(gs=s, dgamma=(gm * h).sum(0), dbeta=gm.sum(0), gm=gm, h=h)


def _close_with_nans(name, got, want, yard, plain):
    """The NaN pattern is the statement's; the finite elements are within max(plain, 4 x yardstick)."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, int(torch.isnan(got).sum()), int(nan.sum()))
    if bool(nan.all()):
        print(f"{name}: NaN throughout, as stated")
        return
    err = float((got.double() - want)[~nan].abs().max())
    yd = float((yard.double() - want)[~nan].abs().max())
    print(f"{name}: kernel {err:.3e} yardstick {yd:.3e} ratio {err / max(yd, 1e-300):.2f} plain {plain:.3e}")
    assert yd > 0
    assert err <= max(plain, 4 * yd), (name, err, yd, plain)


@pytest.mark.parametrize("rows", [37, 16385])
def test_clamp_branch_against_the_float64_rule(rows):
    from egtr_amd import _lib
    x, r, gy, keep, w, b = _inputs(rows, seed=5)
    cv = float(torch.finfo(torch.float32).max - 1000)
    bad_row = rows - 2
    x_inf = x.clone()
    x_inf[bad_row, 5] = float("inf")
    keep[bad_row, 5] = 1
    # the forward raises the flag; the encoder node then clamps y in place and hands it to the backward
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    y_inf = _forward(x_inf, r, keep, SCALE, w, b, flag=flag).clone()
    assert int(flag) == 1 and bool(torch.isnan(y_inf[bad_row]).all())
    assert bool(torch.isfinite(y_inf[torch.arange(rows, device=DEV) != bad_row]).all())
    _lib.launch("egtr_clamp_if_flag_f32", y_inf.data_ptr(), None, y_inf.numel(), flag.data_ptr(), cv, 0)
    n = 2 * math.sqrt(rows) + 32

    def check(tag, xs, y_out):
        gs, gx, gbb = _backward(xs, r, keep, SCALE, w, gy, flag=flag, y_out=y_out, clamp_value=cv)
        ref = _rule(xs, r, gy, keep, w, y_out, cv, torch.float64)
        yard = _rule(xs, r, gy, keep, w, y_out, cv, torch.float32)
        _, s_gs, _ = _row_scales(xs, r, ref["gm"], keep, w)
        finite_rows = ~torch.isnan(ref["gs"]).any(1)
        plain_gs = 64 * U * float(s_gs[finite_rows].max())
        _close_with_nans(f"clamp rows {rows} {tag} grad_sum", gs, ref["gs"], yard["gs"], plain_gs)
        gh = (ref["gm"] * ref["h"])[finite_rows]
        _close_with_nans(f"clamp rows {rows} {tag} d gamma", gbb[:256], ref["dgamma"], yard["dgamma"],
                         n * U * float(gh.abs().sum(0).max()))
        _close_with_nans(f"clamp rows {rows} {tag} d beta", gbb[256:512], ref["dbeta"], yard["dbeta"],
                         n * U * float(ref["gm"].abs().sum(0).max()))
        return ref, gs, gbb

    # 1. as the node runs it: the NaN row passes no incoming gradient (d beta stays finite), its own gradients are NaN
    ref, gs, gbb = check("node", x_inf, y_inf)
    assert bool(torch.isfinite(gbb[256:512]).all()) and bool(torch.isnan(gs[bad_row]).all())
    assert bool(torch.isfinite(gs[torch.arange(rows, device=DEV) != bad_row]).all())
    assert bool((ref["gm"][bad_row] == 0).all())
    # 2. the rule on finite rows: y_out of the clean input with clamped-looking elements planted (+-cv, inf, NaN), flag raised
    y_clean = _forward(x, r, keep, SCALE, w, b).clone()
    planted = y_clean.clone()
    spots = [(0, 0, cv), (0, 255, -cv), (rows // 2, 17, float("inf")), (rows // 2, 18, NAN), (rows - 1, 64, -float("inf")),
             (rows - 1, 200, cv)]
    for row, col, val in spots:
        planted[row, col] = val
    ref, gs, gbb = check("planted", x, planted)
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gbb[:512]).all())
    assert int((ref["gm"] != gy.double()).sum()) == len(spots)
    plain_ref = _rule(x, r, gy, keep, w, y_clean, cv, torch.float64)
    assert float((plain_ref["dbeta"] - ref["dbeta"]).abs().max()) > 0          # (the planted elements carry gradient that shows)
    auto = _compose(x, r, gy, keep, w, b, torch.float64)                            # the written-out rule is LayerNorm's backward
    assert float((plain_ref["gs"] - auto["gs"]).abs().max()) < 1e-12 and float((plain_ref["dgamma"] - auto["dgamma"]).abs().max()) < 1e-10
    # 3. flag at 0: the same call gives the bits of the unclamped call
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _backward(x, r, keep, SCALE, w, gy, flag=zero, y_out=planted, clamp_value=cv)
    u = _backward(x, r, keep, SCALE, w, gy)
    for got, want in zip(a, u):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
