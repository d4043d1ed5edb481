"""Host checks behind tests/test_gpu_decoder_layer.py, with torch on the CPU: the decoders and inputs of
tests/decoder_layer_restated.py can tell a wrong decoder-layer kernel from a right one, and the host helpers that lay the
kernel's operands out (``decoder_fused.pack``, ``_qkv_pack``, ``_rows``) do what the kernel reads.

Resolving power.  The GPU test bounds max |kernel - float64| by 4 x e32 per (output, layer), e32 = the float32 composition's
error.  For every case and every defect of ``DEFECTS`` that can show there, the altered float64 result leaves the reference
by at least 10 x that bound in some compared output.  Smallest defect / bound ratio over all cases, as measured (the case
in brackets):

    b_attn_out dropped                          7579 (large-scores)
    b_cross_out dropped                         4177 (large-scores)
    b_fc1 dropped                               3789 (large-scores)
    b_fc2 dropped                               4295 (large-scores)
    b_qkv_next dropped                          7405 (mask-in-memory-S34000)
    value bias added unweighted                 18475 (large-scores)
    head 5 left out of out_proj                 17220 (large-scores)
    head 2 left out of output_proj              13856 (large-scores)
    a k group left out of fc2                   3111 (large-scores)
    a k group left out of fc1's second half     4864 (large-scores)
    last key left out of the softmax            3771 (large-scores)
    keys >= 256 left out                        24898 (large-scores)
    x and y offsets of one sample swapped       5471 (mask-in-memory-S34000)
    sampling points of two levels swapped       19636 (large-scores)
    padding mask ignored                        18851 (mask-in-memory-S34000)
    image 1 reads image 0's position rows       375809 (loop-B9-N33)
    image 1 reads image 0's reference rows      43422 (mask-in-lds-S32750)
    image 1 reads image 0's padding mask        18851 (mask-in-memory-S34000)
    q of the next layer unscaled                540625 (mask-in-memory-S32770)
    v of the next layer from x + pos            16297 (large-scores)
"""
import pytest
import torch

import decoder_layer_restated as R

@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["name"])
def test_every_defect_leaves_the_reference_by_ten_times_the_bound(c):
    dec, inp = R.build(c)
    ref = R.layer_f64(dec, inp)
    e32 = R.errors(R.layer_f64(dec, inp, dtype=torch.float32), ref)
    assert all(0 < e < 2e-4 for e in e32.values()), e32
    for b, i in R.outside_rows(c):
        assert bool((ref["cross_out"][-1, b, i] == 0).all())
        assert c["layers"] < 2 or float(ref["cross_out"][0, b, i].abs().max()) > 0
    applied = 0
    for name, fn, applies in R.DEFECTS:
        if not applies(c):
            continue
        applied += 1
        moved = R.errors(fn(dec, inp), ref)
        ratio = max(moved[key] / (R.FACTOR * e32[key]) for key in e32)
        print(f"{c['name']}: {name}: {ratio:.0f} x the bound")
        assert ratio >= 10, (c["name"], name, ratio)
    assert applied >= 13


def test_every_defect_can_show_at_some_case():
    assert len(R.DEFECTS) == 20 and len({name for name, _, _ in R.DEFECTS}) == 20
    for name, _, applies in R.DEFECTS:
        assert sum(bool(applies(c)) for c in R.CASES) >= 2, name


def test_the_cases_cover_what_the_issue_lists():
    names = {c["name"]: c for c in R.CASES}
    assert len(names) == len(R.CASES)
    assert {c["N"] for c in R.CASES if c["name"].startswith("edges-B1")} == {1, 7, 8, 9, 63, 64, 65, 256, 257, 320}
    assert {c["N"] for c in R.CASES if c["name"].startswith("edges-B2")} == {1, 7, 8, 9, 63, 64, 65}
    for c in R.CASES:
        if c["name"].startswith("loop"):   # more clusters than the kernel has physical ones, every image's last panel partial
            assert c["B"] * ((c["N"] + 7) // 8) > 32 and c["N"] % 8 and c["mask"] and c["rows"] == "per_image"
    sizes = {n: sum(h * w for h, w in names[n]["levels"]) for n in names if "-S3" in n}
    assert sizes == {"mask-in-memory-S34000": 34000, "mask-in-memory-S32770": 32770, "mask-in-lds-S32750": 32750}
    assert (32770 + 31) // 32 == 1025 and (32750 + 31) // 32 == 1024   # the kernel keeps up to 1024 mask words in LDS
    assert sum(h * w for h, w in R.LEVELS) == 256 and names["depth-6"]["layers"] == 6


def test_no_parameter_is_zero_or_constant_along_columns():
    dec = R.make_decoder(2, 5)
    n = 0
    for name, p in dec.named_parameters():
        n += 1
        assert int((p == 0).sum()) == 0, name
        flat = p.detach().reshape(p.shape[0], -1)
        assert float(flat.std(0).min() if flat.shape[0] > 1 and flat.shape[1] > 1 else flat.std()) > 0, name
        if name.endswith(".bias") and "layer_norm" not in name and "sampling_offsets" not in name:
            assert 0.05 < float(p.detach().std()) < 0.2, name
    assert n == 2 * 26
    a, b = R.make_decoder(2, 5), R.make_decoder(2, 6)
    assert torch.equal(a.layers[1].fc2.weight, dec.layers[1].fc2.weight)
    assert not torch.equal(a.layers[1].fc2.weight, b.layers[1].fc2.weight)
    so = dec.layers[-1].encoder_attn.sampling_offsets.bias.view(8, 4, 4, 2)
    for l, (h, w) in enumerate(R.LEVELS):   # the reserved layer: more than half a level + 3 pixels, in x and in y
        assert float(so.detach()[:, l, :, 0].min()) >= 0.5 * w + 3 and float(so.detach()[:, l, :, 1].min()) >= 0.5 * h + 3
    assert float(dec.layers[0].encoder_attn.sampling_offsets.bias.detach().min()) < -2


def test_inputs_have_the_advertised_form():
    for c in R.CASES:
        if c["levels"] != R.LEVELS:
            continue
        inp = R.make_inputs(c)
        B, N = c["B"], c["N"]
        h, p, ref = inp["hidden_states"], inp["position_embeddings"], inp["reference_input"]
        assert tuple(h.shape) == tuple(p.shape) == (B, N, 256) and tuple(inp["values"].shape) == (c["layers"], B, 256, 256)
        if B > 1:
            assert (h.stride(0) == 0) == (c["rows"] in ("expanded", "mixed")) and (p.stride(0) == 0) == (c["rows"] == "expanded")
            if c["rows"] != "expanded":
                assert not torch.equal(p[0], p[1])
            if c["rows"] == "per_image":
                assert not torch.equal(h[0], h[1])
        pts = ref if c["ref"] == "ratios" else None
        if pts is not None:
            assert tuple(pts.shape) == (B, N, 2) and float(pts.min()) >= 0 and float(pts.max()) <= 1
            for b, i in R.outside_rows(c):
                assert pts[b, i].tolist() == [1.0, 1.0]
            if N >= 64:
                border = ((pts == 0) | (pts == 1)).any(-1).float().mean()
                assert 0.09 < float(border) < 0.16
            vr = inp["valid_ratios"]
            assert tuple(vr.shape) == (B, 4, 2) and float(vr.min()) >= 0.55 and float(vr.max()) <= 1 and bool((vr[0] == 1).all())
            if c["mask"]:
                keep, start = inp["keep_mask"], 0
                assert keep.dtype == torch.bool and bool(keep[0].all()) and (B == 1 or not bool(keep[1:].all()))
                for l, (hh, ww) in enumerate(R.LEVELS):   # bottom and right strips: the valid part is what the ratios say
                    m = keep[:, start:start + hh * ww].view(B, hh, ww)
                    start += hh * ww
                    for b in range(B):
                        vw, vh = round(float(vr[b, l, 0]) * ww), round(float(vr[b, l, 1]) * hh)
                        assert bool(m[b, :vh, :vw].all()) and int(m[b].sum()) == vh * vw
        else:
            assert tuple(ref.shape) == (B, N, 4, 2) and inp["valid_ratios"] is None
        assert (inp["value_bias"] is None) == (not c["bias"]) and (inp["keep_mask"] is None) == (not c["mask"])
        assert (inp["first_with_pos"] is None) == (not c["first_with_pos"])
        if c["first_with_pos"]:
            assert torch.equal(inp["first_with_pos"], h + p)


def test_large_scores_need_the_maximum_and_reach_forty_either_side():
    c = next(c for c in R.CASES if c["name"] == "large-scores")
    dec, inp = R.build(c)
    ref = R.layer_f64(dec, inp)
    for l in range(c["layers"]):
        q = ref["q"][l].view(1, 300, 8, 32).transpose(1, 2)
        k = ref["k"][l].view(1, 300, 8, 32).transpose(1, 2)
        s = q @ k.transpose(-1, -2)
        assert float(s.max()) > 89            # exp() of it overflows float32: the maximum must be subtracted
        spread = s.max(-1).values - s.min(-1).values
        assert float(spread.max()) > 60 and float(spread.median()) > 30   # about +-40 around the shift
    z = ref["states"][0]
    assert torch.isfinite(z).all()


def test_pack_is_the_order_a_wave_consumes_a_tile_in():
    from egtr_amd import decoder_fused
    g = torch.Generator().manual_seed(0)
    for n, k in ((64, 4), (128, 256), (256, 1024), (1024, 256)):
        w = torch.randn(n, k, generator=g)
        p = decoder_fused.pack(w)
        assert tuple(p.shape) == (n // 64, k // 4, 64, 4) and p.is_contiguous()
        for t, k4, c, i in ((0, 0, 0, 0), (n // 64 - 1, k // 4 - 1, 63, 3), ((n // 64) // 2, (k // 4) // 3, 17, 2)):
            assert float(p[t, k4, c, i]) == float(w[64 * t + c, 4 * k4 + i])
        t, k4, c, i = torch.meshgrid(torch.arange(n // 64), torch.arange(k // 4), torch.arange(64), torch.arange(4), indexing="ij")
        assert torch.equal(p, w[64 * t + c, 4 * k4 + i])
    with pytest.raises(AssertionError):
        decoder_fused.pack(torch.zeros(60, 8))


def test_qkv_pack_carries_q_and_k_then_v_and_zeros_per_head():
    from egtr_amd import decoder_fused
    sa = R.make_decoder(2, 3).layers[1].self_attn
    with torch.no_grad():
        tiles, bias = decoder_fused._qkv_pack(sa)
    assert tuple(tiles.shape) == (16, 64, 64, 4) and tuple(bias.shape) == (8 * 128,)
    wq, wk, wv = sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight

    def unpack(tile):   # [64 k4][64 c][4 i] -> [64 c][256 k]
        return tile.permute(1, 0, 2).reshape(64, 256)

    for h in range(8):
        s = slice(32 * h, 32 * h + 32)
        qk, vz = unpack(tiles[2 * h]), unpack(tiles[2 * h + 1])
        assert torch.equal(qk[:32], wq[s]) and torch.equal(qk[32:], wk[s])
        assert torch.equal(vz[:32], wv[s]) and int((vz[32:] != 0).sum()) == 0
        b = bias[128 * h:128 * h + 128]
        assert torch.equal(b[:32], sa.q_proj.bias[s]) and torch.equal(b[32:64], sa.k_proj.bias[s])
        assert torch.equal(b[64:96], sa.v_proj.bias[s]) and int((b[96:] != 0).sum()) == 0


def test_rows_reads_an_expansion_in_place_and_copies_what_the_kernel_cannot_read():
    from egtr_amd import decoder_fused
    g = torch.Generator().manual_seed(1)
    table = torch.randn(20, 256, generator=g)
    t, n = decoder_fused._rows(table.unsqueeze(0).expand(3, 20, 256), 20)
    assert n == 20 and tuple(t.shape) == (20, 256) and t.data_ptr() == table.data_ptr()      # one image's rows, no copy
    fresh = torch.randn(3, 20, 256, generator=g)
    t, n = decoder_fused._rows(fresh, 20)
    assert n == 60 and t.data_ptr() == fresh.data_ptr() and torch.equal(t, fresh.view(60, 256))
    t, n = decoder_fused._rows(fresh[:1], 20)                                                 # a batch of one is not an expansion
    assert n == 20 and t.data_ptr() == fresh.data_ptr()
    wide = torch.randn(3, 20, 300, generator=g)
    view = wide[..., 8:264]                                                                   # non-contiguous rows
    t, n = decoder_fused._rows(view, 20)
    assert n == 60 and t.is_contiguous() and t.data_ptr() % 16 == 0 and torch.equal(t, view.reshape(60, 256))
    buf = torch.randn(3 * 20 * 256 + 4, generator=g)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + 3 * 20 * 256].view(3, 20, 256)                                            # contiguous, 4 bytes off
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    t, n = decoder_fused._rows(off, 20)
    assert n == 60 and t.data_ptr() % 16 == 0 and t.data_ptr() != off.data_ptr() and torch.equal(t, off.view(60, 256))
    points = torch.rand(20, 2, generator=g)                                                   # the reference points go the same way
    t, n = decoder_fused._rows(points.unsqueeze(0).expand(3, 20, 2), 20)
    assert n == 20 and torch.equal(t, points)
