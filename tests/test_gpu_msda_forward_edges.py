"""GPU (-m gpu): every MSDA forward kernel and mask route against the float64 restatement of the fused forward
(tests/msda_forward_restated.py), on operands for which every step of every kernel is exact -- `torch.equal`, for the bf16
kernels with the round-to-nearest-even bfloat16 image of the float64 result -- and, on pyramids that are no powers of two, inside
the element-wise budgets derived there.  tests/test_msda_forward_cases_cpu.py proves on the CPU that each case reaches what it is
named for and that the criteria reject a forward with one piece wrong.

Kernels (csrc/msda.hip) and the cases that run through them:
  msda_fwd_q64_f32<true, true, false / true>   fused, sample-split (B Lq <= 1024), points / boxes: slots, threshold_1024, falloff,
                                               l2p8_37, l1p16_37, one, tiny, odd_37, odd_111, degenerate_37
  msda_fwd_q64_f32<true, false, false / true>  fused, wave per query: slots_wave, threshold_1025, pairs, dense, l2p8_515, l1p16_515,
                                               bits_last_lds, bits_memory, odd_515, degenerate_515
  msda_fwd_q64_f32<false, true> / <false>      plain: the same two lists (the automatic entry resolves to variant 1 for these
                                               shapes, so "auto" and "variant1" are one kernel launched through two entries)
  msda_fwd_generic<float>                      variant 3: every case
  msda_fwd_q32_bf16<false, 4 / 0>              plain bf16: P = 4 cases / l2p8_*, l1p16_* (runtime P = 8, 16)
  msda_fwd_q32_bf16<true, 4 / 0>               fused bf16, bits, packed byte mask, byte mask through the C ABI: likewise
"""
import functools

import pytest
import torch

import hip_test_abi as TA
import msda_forward_restated as FR
import msda_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SMALL = list(FR.EXACT_CASES) + list(FR.ODD_FUSED_CASES)
ALL = SMALL + list(FR.BITS_CASES)


def _kernels():
    from egtr_amd.load_custom import load_hip_kernels
    return load_hip_kernels()


@functools.lru_cache(maxsize=None)
def reference(name, form, mask):
    """With the value bias; FR.without_bias gives the other one.  Built once, left unchanged."""
    x = FR.case(name)
    return FR.reference(x, form, mask=mask, bias=True, geometry=not x["exact"])


def ref_of(name, form, mask, bias):
    r = reference(name, form, mask)
    return r if bias else FR.without_bias(r)


def device_operands(x, bf16=False):
    from egtr_amd.load_custom import pack_keep_bits
    B, S = x["keep"].shape
    fl = (lambda t: t.to(BF)) if bf16 else (lambda t: t)
    d = {n: fl(x[n]).to(DEV) for n in ("value", "ref", "off", "logit")}
    d.update(shapes=x["shapes"].to(DEV), lsi=x["lsi"].to(DEV), keep=x["keep"].to(DEV), vbias=x["vbias"].to(DEV))
    d["bits"] = pack_keep_bits(d["keep"], B, S)
    d["box"] = torch.cat([x["ref"], x["boxwh"]], -1).contiguous().to(DEV)
    # sampling offsets and logits as column blocks of one [B, Lq, 384] tensor (one wider Linear output)
    wide = torch.cat([d["off"].flatten(2), d["logit"].flatten(2)], -1).contiguous()
    d["off_cols"], d["logit_cols"] = wide[..., :256].unflatten(2, x["off"].shape[2:]), wide[..., 256:]
    assert x["off"].shape[1] == 1 or (d["off_cols"].flatten(2).stride(1) == 384 and d["logit_cols"].stride(1) == 384)
    return d


def judge(label, x, got, r, bf16=False):
    """Exact cases: equality with the float64 result (its bfloat16 image); budget cases: worst error-to-bound ratio <= 1."""
    if x["exact"]:
        want = r["out"].to(BF) if bf16 else r["out"].float()
        assert got.dtype == want.dtype
        bad = int((got.cpu() != want).sum())
        assert torch.equal(got.cpu(), want), (label, f"{bad} elements differ")
        return 0.0
    return FR.check(label, got, r, FR.bound_bf16(r) if bf16 else FR.bound_f32(r))


# ----------------------------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("form", ["point", "box"])
@pytest.mark.parametrize("name", ALL)
def test_fused_f32(name, form):
    """ms_deform_attn_forward_fused with 2-d points / 4-d boxes x {no mask, byte mask, keep_bits} x {no bias, value_bias} x
    {contiguous, column blocks}: output, returned weights (exactly 1 / n on the selected slots), and the same bits twice."""
    x = FR.case(name)
    d = device_operands(x)
    k = _kernels()
    weights = reference(name, form, False)["weights"].float()
    for mask in ("none", "bytes", "bits"):
        for bias in (False, True):
            r = ref_of(name, form, mask != "none", bias)
            for cols in (False, True):
                label = f"{name} fused fp32 [{form}, mask {mask}, bias {bias}, {'column blocks' if cols else 'contiguous'}]"
                call = lambda: k.ms_deform_attn_forward_fused(  # noqa: E731
                    d["value"], d["shapes"], d["lsi"], d["off_cols" if cols else "off"], d["logit_cols" if cols else "logit"],
                    d["box" if form == "box" else "ref"], want_weights=True, keep_mask=d["keep"] if mask == "bytes" else None,
                    value_bias=d["vbias"] if bias else None, keep_bits=d["bits"] if mask == "bits" else None)
                out, wts = call()
                torch.cuda.synchronize()
                judge(label, x, out, r)
                assert torch.equal(wts.cpu(), weights), label
                if not cols:
                    again, _ = call()
                    assert torch.equal(again.view(torch.int32), out.view(torch.int32)), (label, "two runs differ")


def _plain_case(name):
    """(host dict, loc, attn, reference): the exact cases hand the prologue's result to the plain entries; the odd pyramids take
    msda_restated.random_case operands (2^-12 location grid) under check_forward's budget."""
    if name in FR.ODD_PLAIN_CASES:
        return _odd_plain(name)
    x = FR.case(name)
    loc, attn = FR.plain_operands(x)
    return x, loc, attn, FR.without_bias(reference(name, "point", False))


@functools.lru_cache(maxsize=None)
def _odd_plain(name):
    x = FR.ODD_PLAIN_CASES[name]()
    x["exact"] = False
    r = R.msda_forward_budget(x["value"], x["pyramid"], x["lsi"].tolist(), x["loc"], x["attn"])
    return x, x["loc"], x["attn"], r


@pytest.mark.parametrize("name", list(FR.EXACT_CASES) + list(FR.BITS_CASES) + list(FR.ODD_PLAIN_CASES))
def test_plain_f32(name):
    """ms_deform_attn_forward (which takes variant 1 for every shape here: the same launch through the product entry) and the
    explicit variants 1 (wave per query / sample split) and 3 (generic)."""
    x, loc, attn, r = _plain_case(name)
    v, sh, lsi, loc, attn = (t.to(DEV) for t in (x["value"], x["shapes"], x["lsi"], loc, attn))
    routes = [("auto", lambda: _kernels().ms_deform_attn_forward(v, sh, lsi, loc, attn, 64)),
              ("variant1", lambda: TA.msda_forward_variant(v, sh, lsi, loc, attn, 1)),
              ("variant3", lambda: TA.msda_forward_variant(v, sh, lsi, loc, attn, 3))]
    for route, call in routes:
        out = call()
        torch.cuda.synchronize()
        if x["exact"]:
            judge(f"{name} plain fp32 [{route}]", x, out, r)
        else:
            R.check_forward(f"{name} plain fp32 [{route}]", out, r)
        assert torch.equal(call().view(torch.int32), out.view(torch.int32)), (name, route, "two runs differ")


# ----------------------------------------------------------------------------------------------------------------- bf16
@pytest.mark.parametrize("name", list(FR.EXACT_CASES) + list(FR.BITS_CASES) + list(FR.ODD_PLAIN_CASES))
def test_plain_bf16(name):
    """ms_deform_attn_forward with a bfloat16 value (fp32 locations and weights)."""
    x, loc, attn, r = _plain_case(name)
    vb = x["value"].to(BF)
    if not x["exact"]:     # the reference of the rounded values
        r = R.msda_forward_budget(vb.float(), x["pyramid"], x["lsi"].tolist(), x["loc"], x["attn"])
        r.update(abs_bias=torch.zeros_like(r["out"]), geo=torch.zeros_like(r["out"]))
    v, sh, lsi, loc, attn = (t.to(DEV) for t in (vb, x["shapes"], x["lsi"], loc, attn))
    out = _kernels().ms_deform_attn_forward(v, sh, lsi, loc, attn, 64)
    torch.cuda.synchronize()
    judge(f"{name} plain bf16", x, out, r, bf16=True)
    again = _kernels().ms_deform_attn_forward(v, sh, lsi, loc, attn, 64)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16)), (name, "two runs differ")


@pytest.mark.parametrize("name", ALL)
def test_fused_bf16(name):
    """ms_deform_attn_forward_fused_bf16 without a mask, with keep_mask (packed by the binding) and with keep_bits, contiguous
    and as column blocks with a row stride of 384 elements; and egtr_msda_forward_fused_bf16 itself with a byte mask."""
    x = FR.case(name)
    d = device_operands(x, bf16=True)
    k = _kernels()
    for mask in ("none", "keep_mask", "keep_bits", "c_abi_bytes"):
        r = ref_of(name, "point", mask != "none", False)
        for cols in (False, True):
            label = f"{name} fused bf16 [mask {mask}, {'column blocks' if cols else 'contiguous'}]"
            if mask == "c_abi_bytes":
                if cols:
                    continue
                call = lambda: TA.msda_forward_fused_bf16_byte_mask(  # noqa: E731
                    d["value"], d["shapes"], d["lsi"], d["off"], d["logit"], d["ref"], d["keep"].to(torch.uint8).contiguous())
            else:
                call = lambda: k.ms_deform_attn_forward_fused_bf16(  # noqa: E731
                    d["value"], d["shapes"], d["lsi"], d["off_cols" if cols else "off"], d["logit_cols" if cols else "logit"],
                    d["ref"], keep_mask=d["keep"] if mask == "keep_mask" else None,
                    keep_bits=d["bits"] if mask == "keep_bits" else None)
            out = call()
            torch.cuda.synchronize()
            judge(label, x, out, r, bf16=True)
            if not cols:
                assert torch.equal(call().view(torch.int16), out.view(torch.int16)), (label, "two runs differ")


# ---------------------------------------------------------------------------------------------------------- containment
def _entries(x, bf16):
    """name -> (form, call(value)) of the wave-per-query kernels on slots_wave (1030 queries)."""
    d = device_operands(x, bf16)
    k = _kernels()
    loc, attn = (t.to(DEV) for t in FR.plain_operands(x))
    if bf16:
        return d, {
            "plain bf16": ("point", lambda v: k.ms_deform_attn_forward(v, d["shapes"], d["lsi"], loc, attn, 64)),
            "fused bf16 bits": ("point", lambda v: k.ms_deform_attn_forward_fused_bf16(
                v, d["shapes"], d["lsi"], d["off"], d["logit"], d["ref"], keep_bits=d["bits"]))}
    return d, {
        "plain fp32": ("point", lambda v: TA.msda_forward_variant(v, d["shapes"], d["lsi"], loc, attn, 1)),
        "fused fp32 bits + bias": ("point", lambda v: k.ms_deform_attn_forward_fused(
            v, d["shapes"], d["lsi"], d["off"], d["logit"], d["ref"], keep_bits=d["bits"], value_bias=d["vbias"])[0]),
        "fused fp32 boxes, byte mask": ("box", lambda v: k.ms_deform_attn_forward_fused(
            v, d["shapes"], d["lsi"], d["off"], d["logit"], d["box"], keep_mask=d["keep"])[0])}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_non_finite_values_stay_in_the_rows_that_read_them(bf16):
    """slots_wave with one NaN and one inf value element (FR.POISON).  The kernels read the four clamped corner addresses of all
    16 records of a (query, head) row whatever the weights -- masked, unselected and out-of-range corners included (0 * NaN) --
    so exactly the rows FR.containment_rows lists turn non-finite in that channel; every other element keeps the bits of the
    clean run.  (bf16: the dot instruction multiplies a channel pair by (weight, 0), so the partner channel of the pair may turn
    NaN as well -- in the same row.)  The model source never reads an out-of-range corner and zeroes padded rows first."""
    x = FR.case("slots_wave")
    d, entries = _entries(x, bf16)
    B, Lq = x["off"].shape[:2]
    bits = torch.int16 if bf16 else torch.int32
    for label, (form, call) in entries.items():
        clean = call(d["value"]).cpu()
        assert bool(torch.isfinite(clean.float()).all())
        dirty_v = d["value"].clone()
        expect = torch.zeros(B, Lq, FR.M, FR.D, dtype=torch.bool)
        partner = torch.zeros_like(expect)
        for b, tok, h, c, what in FR.POISON:
            dirty_v[b, tok, h, c] = what
            rows = FR.containment_rows(x, form, b, tok)[:, h]
            expect[b, :, h, c] |= rows
            partner[b, :, h, c ^ 1] |= rows
        dirty = call(dirty_v).cpu()
        torch.cuda.synchronize()
        nonfinite = ~torch.isfinite(dirty.float()).reshape(expect.shape)
        free = partner & ~expect if bf16 else torch.zeros_like(expect)
        assert bool((nonfinite | free)[expect | free].all()) and bool(nonfinite[expect].all()), (label, "a listed row stayed finite")
        assert not bool(nonfinite[~(expect | free)].any()), (label, "non-finite outside the listed rows")
        same = dirty.view(bits).reshape(expect.shape) == clean.view(bits).reshape(expect.shape)
        assert bool(same[~(expect | free)].all()), (label, "a clean element changed")
        print(f"{label}: {int(expect.sum())} of {expect[..., 0].numel()} rows x 1 channel non-finite, the rest bit-equal")
