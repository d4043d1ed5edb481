"""GPU (-m gpu): the producer's shift + ReLU applied on the halo load of the own 3x3 convolution (egtr_conv3x3_x6_shift_f32,
csrc/conv3x3_x6.hip; ops.conv3x3(..., in_shift=)) and the bottleneck route that uses it (backbone.CONV1_SHIFT_ON_LOAD: conv1 as a
bias-free product, its folded-BN shift + ReLU inside conv2's kernel).

The kernel tests compare against the EXISTING entry on an input that holds relu(x + shift) already: both sides perform the same
single fp32 add and comparison per element before the same split, so the outputs are bit-identical (torch.equal) and no tolerance
applies.  The shift has positive entries in at least half its channels, so a shift leaking into the padding (relu(0 + shift) > 0)
would show on every border output.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SIZES = [(2, 17, 33), (1, 5, 7)]     # ragged tiles in both directions and two images; an image smaller than one tile
C_STRIDE = [(64, 1), (128, 1), (256, 1), (512, 1), (128, 2), (256, 2), (512, 2)]


def _variants(C, stride):
    """every variant the dispatcher serves for (C, stride), with the phase width of its weight stream"""
    from egtr_amd import _lib
    out = []
    for v in range(5):
        if stride == 2 and v > 1:
            break
        if int(_lib.lib().egtr_conv3x3_phase_channels(C, C, stride, v)) > 0:
            out.append(v)
    assert 0 in out
    return out


def _operands(C, size, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = size
    x = torch.randn(B, H, W, C, generator=g).to(DEV).permute(0, 3, 1, 2)        # [B, C, H, W], channels-last memory
    w = (torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(DEV)
    shift = torch.randn(C, generator=g)
    shift[::2] = shift[::2].abs() + 0.25                                        # at least half the entries positive
    return x, w, shift.to(DEV)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C,stride", C_STRIDE)
def test_shift_on_load_is_bit_identical_to_the_existing_entry_on_activated_input(C, stride, size):
    from egtr_amd import ops
    x, w, shift = _operands(C, size, 1000 * C + 10 * stride + size[1])
    assert int((shift > 0).sum()) * 2 >= C
    act = torch.relu(x + shift.view(1, -1, 1, 1)).contiguous(memory_format=torch.channels_last)
    assert ops.conv3x3_supported(x, C, stride) and ops.conv3x3_supported(act, C, stride)
    for v in _variants(C, stride):
        wxs = ops.conv3x3_weights(w, stride, v)
        ref = ops.conv3x3(act, wxs, C, stride, v)
        got = ops.conv3x3(x, wxs, C, stride, v, in_shift=shift)
        assert got.shape == ref.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, ref), f"variant {v}: max |diff| {float((got - ref).abs().max())}"
        # in_shift=None is the existing entry
        raw = ops.conv3x3(x, wxs, C, stride, v)
        assert torch.equal(ops.conv3x3(x, wxs, C, stride, v, in_shift=None), raw)
        assert not torch.equal(raw, ref)


@pytest.mark.parametrize("C,stride", [(64, 1), (128, 2)])
def test_padding_stays_zero_behind_the_activation(C, stride):
    """x = -10: with shift +1 every activated input is 0 and so is every output; with shift +11 every activated input is 1 and the
    output is the existing entry's on an all-ones image -- whose border outputs see the zero padding."""
    from egtr_amd import ops
    g = torch.Generator().manual_seed(7 + C)
    w = (torch.randn(C, C, 3, 3, generator=g).abs() / (9 * C) ** 0.5 + 0.01).to(DEV)   # positive: nothing cancels a leak
    x = torch.full((1, 5, 7, C), -10.0, device=DEV).permute(0, 3, 1, 2)
    ones = torch.ones((1, 5, 7, C), device=DEV).permute(0, 3, 1, 2)
    for v in _variants(C, stride):
        wxs = ops.conv3x3_weights(w, stride, v)
        y0 = ops.conv3x3(x, wxs, C, stride, v, in_shift=torch.full((C,), 1.0, device=DEV))
        assert torch.equal(y0, torch.zeros_like(y0)), f"variant {v}: {int((y0 != 0).sum())} non-zero outputs"
        y1 = ops.conv3x3(x, wxs, C, stride, v, in_shift=torch.full((C,), 11.0, device=DEV))
        ref = ops.conv3x3(ones, wxs, C, stride, v)
        assert torch.equal(y1, ref)
        assert float(ref[0, :, 0, 0].max()) < float(ref[0, :, 1, 1].min())     # (the border does see fewer taps)


@pytest.mark.parametrize("C,stride", [(64, 1), (256, 1), (128, 2)])
def test_non_finite_inputs_reach_exactly_the_outputs_they_reach_in_the_existing_entry(C, stride):
    from egtr_amd import ops
    x, w, shift = _operands(C, (1, 9, 12), 31 + C)
    x = x.clone(memory_format=torch.channels_last)
    x[0, 3, 4, 5] = float("nan")
    x[0, C - 2, 5, 6] = float("inf")
    act = torch.relu(x + shift.view(1, -1, 1, 1)).contiguous(memory_format=torch.channels_last)
    assert int((~torch.isfinite(act)).sum()) == 2          # torch.relu keeps the NaN
    for v in _variants(C, stride):
        wxs = ops.conv3x3_weights(w, stride, v)
        ref = ops.conv3x3(act, wxs, C, stride, v)
        got = ops.conv3x3(x, wxs, C, stride, v, in_shift=shift)
        bad = ~torch.isfinite(ref)
        assert 0 < int(bad.sum()) < bad.numel()
        assert torch.equal(~torch.isfinite(got), bad)
        assert torch.equal(got[~bad], ref[~bad])


@pytest.fixture(scope="module")
def net_and_input():
    import egtr_amd.backbone as bb
    torch.manual_seed(3)
    net = bb.ResNet50Features().to(DEV).eval()
    for m in net.modules():
        if hasattr(m, "running_var"):
            m.running_var.uniform_(0.5, 1.5)
            m.running_mean.normal_(0, 0.1)
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0, 0.1)
    return net, torch.randn(2, 3, 117, 203, device=DEV)


def _blocks(net):
    return [(blk.conv1.in_channels, blk.conv1.out_channels) for li in range(1, 5) for blk in getattr(net, f"layer{li}")]


def test_network_with_shift_on_load_matches_the_epilogue_route(net_and_input, monkeypatch):
    import egtr_amd.backbone as bb
    from egtr_amd import ops
    net, x = net_and_input
    assert bb.CONV1_SHIFT_ON_LOAD is True and bb.CONV2_X6 is True and ops.GEMM_SPLIT_BF16
    assert set(bb.CONV1_PLAIN_SHAPES) <= set(_blocks(net)) and not set(bb.CONV1_PLAIN_SHAPES) & set(bb.CONV1_X6_SHAPES)
    epi, shifted = [], []
    real_addmm, real_conv = torch._addmm_activation, ops.conv3x3
    monkeypatch.setattr(torch, "_addmm_activation",
                        lambda b, a, wt, **k: (epi.append((a.shape[1], wt.shape[1])), real_addmm(b, a, wt, **k))[1])
    monkeypatch.setattr(ops, "conv3x3",
                        lambda *a, **k: (shifted.append(k.get("in_shift") is not None), real_conv(*a, **k))[1])
    vendor = [s for s in _blocks(net) if s not in bb.CONV1_X6_SHAPES]            # 15: all but layer 1 block 0
    with torch.no_grad():
        on = net(x)
        # the epilogue GEMM only for the blocks outside the adopted set; every other conv1's shift rides on its conv3x3
        assert sorted(epi) == sorted(s for s in vendor if s not in bb.CONV1_PLAIN_SHAPES)
        assert len(shifted) == 16 and sum(shifted) == len([s for s in vendor if s in bb.CONV1_PLAIN_SHAPES])
        del epi[:], shifted[:]
        monkeypatch.setattr(bb, "CONV1_SHIFT_ON_LOAD", False)
        off = net(x)
        assert sorted(epi) == sorted(vendor) and len(shifted) == 16 and not any(shifted)
    assert len(on) == len(off) == 3
    for a, b in zip(on, off):
        assert a.shape == b.shape and a.is_contiguous(memory_format=torch.channels_last)
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        print(f"map {tuple(a.shape)}: max |on - off| = {err:.3e}, bound {5e-5 * scale:.3e}")
        assert err < 5e-5 * scale


@pytest.mark.parametrize("switch", ["CONV2_X6", "GEMM_SPLIT_BF16"])
def test_old_route_for_every_block_when_conv2_is_not_the_own_kernel(net_and_input, monkeypatch, switch):
    import egtr_amd.backbone as bb
    from egtr_amd import ops
    net, x = net_and_input
    monkeypatch.setattr(bb if switch == "CONV2_X6" else ops, switch, False)
    epi, shifted = [], []
    real_addmm, real_conv = torch._addmm_activation, ops.conv3x3
    monkeypatch.setattr(torch, "_addmm_activation",
                        lambda b, a, wt, **k: (epi.append((a.shape[1], wt.shape[1])), real_addmm(b, a, wt, **k))[1])
    monkeypatch.setattr(ops, "conv3x3",
                        lambda *a, **k: (shifted.append(k.get("in_shift") is not None), real_conv(*a, **k))[1])
    with torch.no_grad():
        net(x)
    expect = _blocks(net) if switch == "GEMM_SPLIT_BF16" else [s for s in _blocks(net) if s not in bb.CONV1_X6_SHAPES]
    assert sorted(epi) == sorted(expect) and not shifted
