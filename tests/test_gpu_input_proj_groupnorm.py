"""GPU (-m gpu): the input-projection epilogue (egtr_amd/csrc/elementwise.hip: gn_stats_levels / gn_apply_flatten and
gn_partial_tokens / gn_finalize_tokens / gn_apply_tokens) through its five entries -- flatten f32 / bf16, tokens f32 / bf16,
token slabs f32 -- against the float64 restatement and the per-output bound of tests/groupnorm_restated.py, which is derived
from the operation: an entry passes when every output is as good as an fp32 evaluation with exact statistics can be (and, for
bf16, one more rounding to nearest).

The cases (groupnorm_restated.TOKEN_CASES, NCHW_CASES, SLAB_CASES; tests/test_groupnorm_cases_cpu.py shows for every one of
them that torch's fp32 group_norm is inside the bound and that the single-pass fp32 statistics these kernels used to compute
are not, on the cancelling family) are the smallest that run every loop past its first round: 1, 7, 255, 256, 257 tokens,
2049 (9 chunks: the second round of the finalize loop) and 2305; planes of 1, 31..33, 1023..1025 (the unrolled loads u >= 1)
and 8192, 8193 pixels (the second i0 round); 1 to 4 levels with 1 and 3 images (unused level slots are filled from level 0);
slabs in 1, 2, 8, 9, 10, 16, 17 and 36 pieces (all four workgroup sizes, a second round of the 8-slab loop, 9 partials on 70
tokens).  Families: benign, offset (group mean / std 0, 3, 30, 300), constant (variance 0), tiny_var (eps dominates), scales
(1e-3 .. 1e3); levels differ in parameters and, in the mixed cases, in distribution, so a level-slot mix-up is O(1).

The wrappers allocate ``out`` themselves, so that a level's tokens do not leak into its neighbour's rows is checked on the rows
either side of every level boundary against the reference."""
import pytest
import torch
import torch.nn as nn

import groupnorm_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ids(cases):
    return [c.id for c in cases]


def _projs(d, channels=256, groups=32):
    projs = nn.ModuleList([nn.Sequential(nn.Conv2d(8, channels, 1), nn.GroupNorm(groups, channels, eps=R.EPS)) for _ in d.x])
    with torch.no_grad():
        for p, cb, g, b in zip(projs, d.bias, d.gamma, d.beta):
            p[0].bias.copy_(cb[:channels])
            p[1].weight.copy_(g[:channels])
            p[1].bias.copy_(b[:channels])
    if d.case.bf16:       # the data's parameters are bf16 values already: the entries widen them back to these
        projs = projs.bfloat16()
    return projs.to(DEV)


def _check(d, got, what):
    case = d.case
    ref, bound = d.reference()
    assert got.shape == ref.shape and got.dtype == (torch.bfloat16 if case.bf16 else torch.float32)
    g = got.cpu().double()
    assert bool(torch.isfinite(g).all()), what
    q = R.worst_ratio(g, ref, bound, case.bf16)
    print(f"\n[{case.id}] {what}: worst err / bound {q:.3f}, max |err| {float((g - ref).abs().max()):.3g}")
    # the rows either side of every level boundary, on their own: a token written into the neighbouring level's rows
    start = 0
    for T in case.tokens[:-1]:
        start += T
        rows = slice(start - 1, start + 1)
        assert R.worst_ratio(g[:, rows], ref[:, rows], bound[:, rows], case.bf16) <= 1.0, (what, "level boundary", start)
    assert q <= 1.0, what
    return q


# ---- token-major entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TOKEN_CASES, ids=_ids(R.TOKEN_CASES))
def test_token_entry_against_float64(case):
    from egtr_amd import ops
    d = R.build(case)
    projs = _projs(d)
    xs = [x.to(DEV) for x in d.x]
    with torch.no_grad():
        got = ops.input_proj_groupnorm_tokens(xs, projs)
        again = ops.input_proj_groupnorm_tokens(xs, projs)
    assert torch.equal(got, again), "two calls on the same input must be bit-identical"
    _check(d, got, "tokens")


# ---- NCHW entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.NCHW_CASES, ids=_ids(R.NCHW_CASES))
def test_nchw_entry_against_float64_and_the_token_entry(case):
    from egtr_amd import ops
    d = R.build(case)
    projs = _projs(d)
    xs = [x.to(DEV) for x in d.x]
    with torch.no_grad():
        got = ops.input_proj_groupnorm_flatten(xs, projs)
        again = ops.input_proj_groupnorm_flatten(xs, projs)
    assert torch.equal(got, again), "two calls on the same input must be bit-identical"
    _check(d, got, "flatten")
    if not case.bf16:
        with torch.no_grad():
            tok = ops.input_proj_groupnorm_tokens([x.flatten(2).transpose(1, 2).contiguous() for x in xs], projs)
        dd = float((got - tok).abs().max())
        print(f"[{case.id}] max |flatten - tokens| {dd:.3g}")
        assert dd < 2e-5


# ---- slab entry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SLAB_CASES, ids=_ids(R.SLAB_CASES))
def test_slab_entry_against_float64_of_the_in_order_sum(case):
    """The reference takes the fp32 in-order slab sum; that the kernel forms exactly that sum is the bit-equality of slab 0."""
    from egtr_amd import ops
    d = R.build(case)
    projs = _projs(d)
    work = [s.to(DEV) for s in d.slabs]
    twin = [s.to(DEV) for s in d.slabs]
    with torch.no_grad():
        got = ops.input_proj_groupnorm_token_slabs(work, projs)
        again = ops.input_proj_groupnorm_token_slabs(twin, projs)
    assert torch.equal(got, again), "two calls on the same slabs must be bit-identical"
    for wk, sl, s32 in zip(work, d.slabs, d.x):
        assert torch.equal(wk[0].cpu(), s32), "slab 0 must hold the sum in slab order"
        if sl.shape[0] > 1:
            assert torch.equal(wk[1:].cpu(), sl[1:]), "slabs 1 .. S - 1 must be left as they were"
    _check(d, got, "token slabs")
    if all(S == 1 for S in case.splits):
        with torch.no_grad():
            plain = ops.input_proj_groupnorm_tokens([x.to(DEV) for x in d.x], projs)
        assert torch.equal(got, plain), "with S = 1 this is the plain entry, bit for bit"


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _small(entry, levels=2, bf16=False):
    sizes = [(3, 5), (2, 2), (1, 3), (2, 1), (1, 1)] if entry == "nchw" else [15, 4, 3, 2, 1]
    case = R.GnCase(entry, sizes[:levels], 1, ["benign"] * levels, bf16=bf16, splits=[2] * levels if entry == "slabs" else None,
                    tag="-refusal")
    return R.build(case)


def _call(entry, xs, projs):
    from egtr_amd import ops
    fn = {"tokens": ops.input_proj_groupnorm_tokens, "nchw": ops.input_proj_groupnorm_flatten,
          "slabs": ops.input_proj_groupnorm_token_slabs}[entry]
    with torch.no_grad():
        return fn(xs, projs)


def _inputs(d):
    return [s.to(DEV) for s in (d.slabs if d.case.entry == "slabs" else d.x)]


@pytest.mark.parametrize("entry", ["tokens", "nchw", "slabs"])
def test_refusals_stay_refusals(entry):
    from egtr_amd._lib import EgtrHipError
    refused = (ValueError, EgtrHipError)
    d = _small(entry)
    projs = _projs(d)
    _check(d, _call(entry, _inputs(d), projs), f"{entry}, the accepted twin")
    # a level of 0 tokens
    xs = _inputs(d)
    empty = {"tokens": (1, 0, 256), "nchw": (1, 256, 0, 3), "slabs": (2, 1, 0, 256)}[entry]
    with pytest.raises(refused):
        _call(entry, [xs[0], torch.empty(empty, device=DEV)], projs)
    # 5 levels
    d5 = _small(entry, levels=5)
    with pytest.raises(refused):
        _call(entry, _inputs(d5), _projs(d5))
    # C != 256
    narrow = {"tokens": lambda x: x[..., :128].contiguous(), "nchw": lambda x: x[:, :128].contiguous(),
              "slabs": lambda x: x[..., :128].contiguous()}[entry]
    with pytest.raises(refused):
        _call(entry, [narrow(x) for x in xs], _projs(d, channels=128))
    # groups != 32: the token kernels are written for 8 channels per group (the NCHW kernel takes any divisor of 256)
    if entry != "nchw":
        with pytest.raises(refused):
            _call(entry, xs, _projs(d, groups=16))
