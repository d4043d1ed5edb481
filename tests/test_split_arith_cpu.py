"""The host restatement of the split-bf16 arithmetic (tests/helpers.py) that tests/test_gpu_backbone_x6.py measures the backbone
kernels with: the two splits, the XS layout decoder, and the property of the paired operand families that lets one lost product
term be told from accumulation noise.  No kernel runs here."""
import numpy as np
import pytest
import torch

import helpers as H


def _wide_values():
    """fp32 values at every binade 2^-120 .. 2^120 with random mantissas, the fp32 denormals, zeros and the largest finites."""
    g = torch.Generator().manual_seed(11)
    e = torch.arange(-120, 121, dtype=torch.float64).repeat_interleave(64)
    m = (1 + torch.rand(e.numel(), generator=g, dtype=torch.float64)) * torch.where(torch.rand(e.numel(), generator=g) < 0.5, -1.0, 1.0)
    normal = (m * torch.pow(2.0, e)).float()
    den_bits = torch.randint(1, 1 << 23, (4096,), generator=g)
    den_bits[:4] = torch.tensor([1, 2, 0x7fffff, 0x400000])
    den = H._bits_f32(den_bits | (torch.randint(0, 2, (4096,), generator=g) << 31))
    edge = torch.tensor([0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 2.0 ** -126, 2.0 ** -110, 1.0, 1.0 + 2.0 ** -23,
                         1.99999988079071044921875, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23], dtype=torch.float32)
    return torch.cat([normal, den, edge])


def _is_bf16(t):
    return bool(((H._f32_bits(t) & 0xffff) == 0).all())


def test_split_helpers_are_exact_three_way_bf16_splits():
    """Truncation: every piece a bf16, |lo| < 2^-15 |x| (lo holds at most the last 8 of x's 24 bits, 2^(e-16) .. 2^(e-23) with
    2^e <= |x|; x = 1 + 2^-8 + 2^-16 + 2^-23 has lo = 2^-16 + 2^-23 > 2^-16 x, so the factor cannot be 2^-16), and
    hi + mid + lo == x exactly wherever three bf16 CAN hold x, i.e.
    while x's last bit is not below the bf16 format's smallest step 2^-133 (|x| >= 2^-110); below that, fp32 denormals
    included, what is lost is less than that one step.  To nearest even: every piece a bf16, the sum within 2^-24 |w| (three
    roundings to 8 bits each) or half the smallest step per rounding, 2^-134, whichever is larger; pieces in descending order."""
    x = _wide_values()
    xd = x.double()
    hi, mid, lo = H.split3_trunc(x)
    assert _is_bf16(hi) and _is_bf16(mid) and _is_bf16(lo)
    s = hi.double() + mid.double() + lo.double()
    big = xd.abs() >= 2.0 ** -110
    assert int(big.sum()) > 64 * 200 and int((~big).sum()) > 4096
    assert torch.equal(s[big], xd[big])
    assert bool(((xd - s).abs() < 2.0 ** -133).all())
    assert bool((lo.double().abs() <= 2.0 ** -15 * xd.abs()).all())
    assert float(H.split3_trunc(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23]))[2]) == 2.0 ** -16 + 2.0 ** -23
    assert bool((mid.double().abs() <= 2.0 ** -7 * hi.double().abs()).all())      # a truncation residual is below one 8-bit step
    assert bool((lo.double().abs() <= 2.0 ** -7 * mid.double().abs()).all())
    assert bool((hi.double().abs() <= xd.abs()).all()) and bool((torch.sign(hi) * torch.sign(x) >= 0).all())

    hi, mid, lo = H.split3_rne(x)
    assert _is_bf16(hi) and _is_bf16(mid) and _is_bf16(lo)
    fin = torch.isfinite(hi)                                                         # the largest finites round up to inf
    assert int((~fin).sum()) == 2
    s = hi.double() + mid.double() + lo.double()
    err = (xd - s).abs()[fin]
    assert bool((err <= torch.clamp(2.0 ** -24 * xd.abs()[fin], min=2.0 ** -134)).all())
    assert torch.equal(s[big & fin], xd[big & fin])                                  # nothing is lost in the normal range either
    assert bool((mid.double().abs() <= 2.0 ** -8 * hi.double().abs())[fin].all())   # a rounding residual is at most half a step
    assert bool((lo.double().abs() <= 2.0 ** -8 * mid.double().abs())[fin].all())
    # the rounding itself against torch's own fp32 -> bf16 conversion (round to nearest even)
    assert torch.equal(hi[fin], x.bfloat16().float()[fin])


def test_split_helpers_non_finite_values_stay_in_the_leading_piece():
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.5])
    for split in (H.split3_trunc, H.split3_rne):
        hi, mid, lo = split(x)
        assert torch.equal(hi[:2], x[:2]) and bool(torch.isnan(hi[2])) and float(hi[3]) == 1.5
        assert torch.equal(mid, torch.zeros(4)) and torch.equal(lo, torch.zeros(4))


@pytest.mark.parametrize("rows,K", [(1, 16), (37, 48), (64, 32)])
def test_xs_decode_reads_a_stream_written_element_by_element(rows, K):
    """The decoder against an encoder that places every bf16 by the format description, one element at a time."""
    g = torch.Generator().manual_seed(rows + K)
    pieces = [H._trunc_bf16(torch.randn(rows, K, generator=g)) for _ in range(3)]
    n = ((rows + 31) // 32) * (K // 16) * 3 * 1024
    buf = np.full(n, 0xAB, dtype=np.uint8)                                          # rows beyond the matrix: never read
    for p, t in enumerate(pieces):
        bits = (H._f32_bits(t) >> 16).numpy()
        for row in range(rows):
            for k in range(K):
                frag = ((row // 32) * (K // 16) + k // 16) * 3 + p
                byte = frag * 1024 + ((k % 16) // 8) * 512 + (row % 32) * 16 + (k % 8) * 2
                buf[byte], buf[byte + 1] = bits[row, k] & 0xff, bits[row, k] >> 8
    got = H.xs_decode(torch.from_numpy(buf), rows, K)
    assert all(torch.equal(a, b) for a, b in zip(got, pieces))


def _chained_fp32(a_pieces, w_pieces):
    """The pessimistic accumulation model: per 16-k step the six terms in x6::mfma6's order, every single product (exact in fp32:
    two 8-bit factors) added to ONE fp32 accumulator in turn -- a chain of 6 K roundings per output."""
    M, K = a_pieces[0].shape
    acc = torch.zeros(M, w_pieces[0].shape[0])
    for k0 in range(0, K, 16):
        for wi, ai in H.SIX_TERMS:
            for k in range(k0, k0 + 16):
                acc += a_pieces[ai][:, k:k + 1] * w_pieces[wi][:, k].unsqueeze(0)
    return acc


@pytest.mark.parametrize("family", ["act", "wgt"])
@pytest.mark.parametrize("K", [64, 576, 2304, 4608])
def test_paired_operands_separate_a_lost_term_from_accumulation_noise(family, K, capsys):
    """For the committed generators: the six-term sum is >= 50x closer to the fp64 product than a five-term sum without either
    of the two small terms the family resolves, and both the harshest accumulation model of a correct kernel and a plain fp32
    product stay under the geometric mean of the two -- the bar the GPU tests hold the kernels to -- at every K the backbone
    has.  The family's third small term is exactly zero by construction (its pieces cancel within a pair), so the other family
    has to resolve it: between them the two cover w_lo a_hi, w_hi a_lo and w_mid a_mid."""
    gen = torch.Generator().manual_seed(100 * K + len(family))
    a, w = H.paired_operands(family, (256, K), (64, K), gen)
    op = lambda x, y: x @ y.t()
    ref, e_model, e_loss = H.split_error_model(op, a, w, lost=H.RESOLVED_TERMS[family])
    (blind,) = [t for t in H.SMALL_TERMS if t not in H.RESOLVED_TERMS[family]]
    ap, wp = H.split3_trunc(a), H.split3_rne(w)
    assert float(H.term_sum(op, ap, wp, [blind]).abs().max()) == 0.0
    assert sorted(set(H.RESOLVED_TERMS["act"]) | set(H.RESOLVED_TERMS["wgt"])) == sorted(H.SMALL_TERMS)
    bar = (e_model * e_loss) ** 0.5
    e_chain = H.rel_fro(_chained_fp32(ap, wp), ref)
    e_mm = H.rel_fro(a @ w.t(), ref)
    with capsys.disabled():
        print(f"\n[paired {family} K={K}] E_model {e_model:.3g}  chained fp32 {e_chain:.3g}  fp32 mm {e_mm:.3g}  "
              f"E_loss {e_loss:.3g}  bar {bar:.3g}")
    assert e_loss >= 50 * e_model
    assert e_chain <= bar and e_mm <= bar
    # the leading products cancel: the result is small against sum |a| |w|
    assert float(ref.abs().max()) < 2.0 ** -6 * float((a.double().abs() @ w.double().abs().t()).max())


# ---- the extensions tests/test_gpu_token_x6.py needs ------------------------------------------------------------------------------
def _health(op, a, w, family, post=None, **splits):
    ref, e_model, e_loss = H.split_error_model(op, a, w, post=post, lost=H.RESOLVED_TERMS[family], **splits)
    (blind,) = [t for t in H.SMALL_TERMS if t not in H.RESOLVED_TERMS[family]]
    ap = splits.get("a_split", H.split3_trunc)(a)
    wp = splits.get("w_split", H.split3_rne)(w)
    assert float(H.term_sum(op, ap, wp, [blind]).abs().max()) == 0.0           # the third small term: exactly zero
    return ref, e_model, e_loss


@pytest.mark.parametrize("family", ["act", "wgt"])
@pytest.mark.parametrize("K", [32, 256, 1024])
def test_non_negative_paired_operands_resolve_the_same_terms(family, K, capsys):
    """The non-negative variant (activations behind a ReLU): a >= 0 everywhere, relu(a) == a, and the same separation
    E_loss >= 50 E_model with the same third small term exactly zero as the signed families; the fp32 product under the bar."""
    op = lambda x, y: x @ y.t()
    gen = torch.Generator().manual_seed(7 * K + len(family))
    a, w = H.paired_operands(family, (200, K), (64, K), gen, nonneg=True)
    assert bool((a >= 0).all()) and torch.equal(torch.relu(a), a)
    if family == "wgt":
        assert torch.equal(a[:, 1::2], a[:, 0::2])
        assert torch.equal(H.split3_rne(w[:, 1::2].contiguous())[0], -H.split3_rne(w[:, 0::2].contiguous())[0])
    ref, e_model, e_loss = _health(op, a, w, family)
    bar = (e_model * e_loss) ** 0.5
    with capsys.disabled():
        print(f"\n[paired nonneg {family} K={K}] E_model {e_model:.3g} E_loss {e_loss:.3g} bar {bar:.3g}")
    assert e_loss >= 50 * e_model
    assert H.rel_fro(a @ w.t(), ref) <= bar
    assert float(ref.abs().max()) < 2.0 ** -6 * float((a.double() @ w.double().abs().t()).max())


@pytest.mark.parametrize("family", ["act", "wgt"])
@pytest.mark.parametrize("M", [34, 778, 4100])
def test_truncation_truncation_family_of_the_weight_gradient(family, M, capsys):
    """g^T x with both operands split by truncation, pairs along the reduction index m (adjacent rows): the split function per
    operand of ``split_error_model``, E_loss >= 50 E_model, the third small term exactly zero, both families."""
    gen = torch.Generator().manual_seed(M + len(family))
    gt, xt = H.paired_operands_trunc(family, (128, M), (128, M), gen)           # [N, M], [K, M]
    g, x = gt.t().contiguous(), xt.t().contiguous()
    op = lambda gg, xx: gg.t() @ xx
    both = dict(a_split=H.split3_trunc, w_split=H.split3_trunc)
    ref, e_model, e_loss = _health(op, g, x, family, **both)
    shared = x if family == "wgt" else g
    assert torch.equal(H.split3_trunc(shared[1::2].contiguous())[0], H.split3_trunc(shared[0::2].contiguous())[0])
    bar = (e_model * e_loss) ** 0.5
    with capsys.disabled():
        print(f"\n[paired trunc {family} M={M}] E_model {e_model:.3g} E_loss {e_loss:.3g} bar {bar:.3g}")
    assert e_loss >= 50 * e_model
    assert H.rel_fro(g.t() @ x, ref) <= bar
    # the default splits are still activation = truncation, weight = nearest even
    d = H.split_error_model(op, g, x, lost=H.RESOLVED_TERMS[family])
    e = H.split_error_model(op, g, x, lost=H.RESOLVED_TERMS[family], a_split=H.split3_trunc, w_split=H.split3_rne)
    assert d[1:] == e[1:]


def test_add_on_load_decomposition_is_exact():
    """x = a_hi + a_mid, pos = a_lo: the fp32 sum x + pos is a bit for bit, for every value three bf16 can hold; below 2^-110
    (a paired partner of an activation that is exactly zero is an fp32 denormal) pos = a - x keeps the sum exact as well."""
    a = _wide_values()
    x, pos = H.add_on_load(a)
    assert torch.equal(H._f32_bits(x + pos), H._f32_bits(a + 0.0))
    full = a.abs() >= 2.0 ** -110
    assert float(pos[full].abs().max()) > 0 and _is_bf16(pos[full]) and torch.equal(pos[full], H.split3_trunc(a)[2][full])
    g = torch.Generator().manual_seed(4)
    a, _ = H.paired_operands("act", (37, 64), (8, 64), g)
    x, pos = H.add_on_load(a)
    assert torch.equal(H._f32_bits(x + pos), H._f32_bits(a))


def test_selector_and_identity_weights_return_the_activation_exactly():
    """A 0 / 1 weight is (1, 0, 0) in pieces, so its six-term product is a_hi + a_mid + a_lo (and zeros) added in fp32 in SOME
    order.  Every partial sum of the pieces of one fp32 number is representable -- hi + mid is the leading 16 bits, hi + lo and
    mid + lo fit in 24 bits between the first bit of the larger and the last bit of a -- so every order returns a exactly."""
    import itertools
    a = _wide_values()
    a = a[(a.abs() >= 2.0 ** -110) & (a.abs() < 2.0 ** 120)]
    one = torch.ones(1)
    assert [float(p) for p in H.split3_rne(one)] == [1.0, 0.0, 0.0]
    pieces = H.split3_trunc(a)
    for order in itertools.permutations(range(3)):
        acc = torch.zeros_like(a)
        for i in order:
            acc = acc + pieces[i] * one                                          # the product with 1 is exact
            acc = acc + 0.0 * pieces[i]                                          # the terms with the weight's zero pieces
        assert torch.equal(H._f32_bits(acc), H._f32_bits(a + 0.0)), order
    # as a matrix: a selector of a window of the hidden layer after the ReLU
    g = torch.Generator().manual_seed(9)
    h, _ = H.paired_operands("wgt", (37, 64), (8, 64), g, nonneg=True)
    sel = torch.zeros(16, 64)
    sel[torch.arange(16), 32 + torch.arange(16)] = 1.0
    six = H.term_sum(lambda x, y: x @ y.t(), H.split3_trunc(h), H.split3_rne(sel), H.SIX_TERMS)
    assert torch.equal(six, h[:, 32:48].double())
