"""No GPU: every case that tests/test_gpu_input_proj_groupnorm.py runs, checked for what the GPU file takes for granted
(tests/groupnorm_restated.py):

* torch's own fp32 group_norm on the same fp32 inputs stays inside the per-output bound -- the bound is one that a plain fp32
  implementation meets, on every case, the cancelling ones included;
* the float64 result rounded to bf16 is inside the bf16 bar;
* the input families have the ratios, zero variances and magnitudes they claim;
* the single-pass fp32 statistics the kernels used to compute (per-thread fp32 partial sums, E[v^2] - mean^2) leave the bound on
  the cancelling family, in the token kernels' order and in the NCHW kernel's, and stay inside it on the benign one: the bound
  has teeth exactly where the old arithmetic was wrong.

Figures on the committed data: torch fp32 at most 0.951 of the bound over the 89 cases; the old accumulation 4.5 .. 1286 x
outside on the groups at ratio >= 30 of every offset case (token order 10 .. 1286, NCHW order 4.5 .. 286), 0.12 .. 0.97 on the
benign ones.  torch evaluates x (r gamma) + (beta - m r gamma), whose worst case equals the bound where v = m: the first
condition is one about torch's VECTORISED CPU kernels on this data (groupnorm_restated.GnCase.salt); its scalar path
(ATEN_CPU_CAPABILITY=default) adds the statistics up differently and is outside on 18 cases, up to 1.47."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_restated as R

IDS = [c.id for c in R.ALL_CASES]


def test_case_ids_are_unique_and_the_lists_cover_what_they_promise():
    assert len(set(IDS)) == len(IDS)
    tok = {t for c in R.TOKEN_CASES for t in c.tokens}
    assert {1, 7, 255, 256, 257, 2049, 2305} <= tok
    for bf16 in (False, True):
        assert {(len(c.sizes), c.B) for c in R.TOKEN_CASES if c.bf16 == bf16} >= {(L, B) for L in (1, 2, 3, 4) for B in (1, 3)}
        assert {t for c in R.NCHW_CASES if c.bf16 == bf16 for t in c.tokens} >= set(R.NCHW_PLANES)
        for entry in (R.TOKEN_CASES, R.NCHW_CASES):
            assert {f for c in entry if c.bf16 == bf16 and c.tag == "-fam" for f in c.families} == set(R.FAMILIES)
    assert {f for c in R.SLAB_CASES if c.tag == "-fam" for f in c.families} == set(R.FAMILIES)
    assert {s for c in R.SLAB_CASES for s in c.splits} == {1, 2, 8, 9, 10, 16, 17, 36}
    assert {t for c in R.SLAB_CASES for t in c.tokens} == {5, 31, 32, 33, 70}
    assert {c.B for c in R.SLAB_CASES} == {1, 2}
    assert [36, 1, 9, 17] in [c.splits for c in R.SLAB_CASES]
    # 8-token workgroups on 70 tokens: 9 partials, the second round of the finalize loop
    assert any(S > 16 and t == 70 for c in R.SLAB_CASES for S, t in zip(c.splits, c.tokens))
    assert [R.slab_chunk_tokens(S) for S in (1, 2, 8, 9, 16, 17, 36)] == [256, 32, 32, 16, 16, 8, 8]


def _torch_fp32(d):
    outs = []
    for x, cb, g, b in zip(d.x, d.bias, d.gamma, d.beta):
        # [B, 256, T] for either layout: a [B, 256, 1, 1] plane is channels-last as well as contiguous to torch, and its
        # channels-last CPU path takes E[v^2] - mean^2 in fp32 (97 x the bound at ratio 300)
        x32 = x.float().transpose(1, 2) if d.layout == "tokens" else x.float().flatten(2)
        v = (x32 + cb.view(1, -1, 1)).contiguous()                    # the bias added in fp32
        outs.append(F.group_norm(v, R.GROUPS, g, b, R.EPS).transpose(1, 2))
    return torch.cat(outs, 1)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=IDS)
def test_reference_alone_is_inside_the_bar_and_the_family_is_what_it_claims(case):
    d = R.build(case)
    for fam, x, cb, T in zip(case.families, d.x, d.bias, case.tokens):
        xt = x.flatten(2).transpose(1, 2) if d.layout == "nchw" else x
        R.check_family(fam, xt, cb, case.bf16, T)
    ref, bound = d.reference()
    assert ref.shape == (case.B, sum(case.tokens), R.C) and bool(torch.isfinite(ref).all()) and bool((bound > 0).all())
    q = R.worst_ratio(_torch_fp32(d), ref, bound)
    print(f"\n[{case.id}] torch fp32 group_norm: worst err / bound {q:.3f}")
    assert q <= 1.0
    if case.bf16:
        qb = R.worst_ratio(ref.bfloat16(), ref, bound, bf16=True)
        assert qb <= 1.0, qb


def _old(d, order):
    ct = [R.slab_chunk_tokens(S) for S in d.case.splits] if d.case.entry == "slabs" else None
    return R.restate_single_pass_fp32(d.x, d.bias, d.gamma, d.beta, R.EPS, d.layout, order=order, chunk_tokens=ct)


def _ratio_by_group(got, ref, bound, bf16):
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / R.bar(ref, bound, bf16))
    return q.view(q.shape[0], q.shape[1], R.GROUPS, R.CPG).amax((0, 1, 3))


@pytest.mark.parametrize("case", [c for c in R.ALL_CASES if set(c.families) == {"offset"}],
                         ids=[c.id for c in R.ALL_CASES if set(c.families) == {"offset"}])
def test_old_single_pass_fp32_statistics_leave_the_bound_on_the_offset_family(case):
    """The old accumulation in the order of the case's own kernel, and the fp32 cases in the other kernel's order as well.
    Judged where the old arithmetic is claimed wrong: on the groups at ratio >= 30 (the NCHW order is still inside at 3)."""
    d = R.build(case)
    ref, bound = d.reference()
    hot = [g for g in range(R.GROUPS) if R.OFFSET_RATIOS[g % 4] >= 30]
    orders = [d.layout] if case.bf16 else ["tokens", "nchw"]
    for order in orders:
        q = _ratio_by_group(_old(d, order), ref, bound, case.bf16)
        print(f"\n[{case.id}] old accumulation, {order} order: worst err / bound at ratio >= 30: {float(q[hot].max()):.1f}, "
              f"at ratio 3: {float(q[1::4].max()):.2f}, at ratio 0: {float(q[0::4].max()):.2f}")
        assert float(q[hot].max()) > 1.0, order


@pytest.mark.parametrize("case", [c for c in R.ALL_CASES if set(c.families) == {"benign"}],
                         ids=[c.id for c in R.ALL_CASES if set(c.families) == {"benign"}])
def test_old_single_pass_fp32_statistics_stay_inside_the_bound_on_the_benign_family(case):
    d = R.build(case)
    ref, bound = d.reference()
    q = R.worst_ratio(_old(d, d.layout), ref, bound, case.bf16)
    print(f"\n[{case.id}] old accumulation on benign data: worst err / bound {q:.3f}")
    assert q <= 1.0


def test_double_accumulation_in_the_kernels_order_is_inside_the_bound_at_every_ratio():
    """what the kernels do now, emulated: the same thread order with every element added in float64"""
    case = next(c for c in R.TOKEN_CASES if c.tokens == [257] and not c.bf16)
    d = R.build(case)
    ref, bound = d.reference()
    x, cb = d.x[0].double(), d.bias[0].double()
    v = (x + cb).view(case.B, -1, R.GROUPS, R.CPG)
    mean = v.sum((1, 3)) / (v.shape[1] * R.CPG)
    var = ((v * v).sum((1, 3)) / (v.shape[1] * R.CPG) - mean * mean).clamp_min(0.0)
    m32 = mean.float().repeat_interleave(R.CPG, 1)[:, None]
    r32 = (1.0 / (var + R.EPS).sqrt()).float().repeat_interleave(R.CPG, 1)[:, None]
    got = ((d.x[0] + d.bias[0]) - m32) * r32 * d.gamma[0] + d.beta[0]
    q = R.worst_ratio(got, ref, bound)
    print(f"\n[{case.id}] E[v^2] - mean^2 with float64 sums, applied in fp32: worst err / bound {q:.3f}")
    assert q <= 1.0
