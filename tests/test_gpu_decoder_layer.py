"""GPU (-m gpu): the one-launch decoder layer (csrc/dec_layer.hip, ``egtr_decoder_layer_f32``) through
``decoder_fused.run`` against a float64 restatement of the layer stack (tests/decoder_layer_restated.py) -- the states of
every layer and the scaled q / k of every layer, every element -- on decoders whose every bias and column matters, at the
row-panel and key-tile edges, with cluster loops that cross images, every row source, both forms of the reference points,
with and without value bias and padding mask, the mask held in LDS and read from memory, large shifted scores, six layers.

Bound: max |kernel - float64| <= 4 x e32 per (output, layer), e32 = the error of the SAME composition run in float32 on the
CPU, computed per case.  tests/test_decoder_layer_inputs_cpu.py shows every listed defect at least 10x above that bound.

Measured kernel error / e32 on an MI355X, the largest (output[layer]) of each case -- the bound is 4, the largest seen 1.69:

    edges-B1-N1                      1.69 (k[1])
    edges-B1-N7                      1.20 (q[1])
    edges-B1-N8                      1.22 (states[1])
    edges-B1-N9                      1.53 (k[1])
    edges-B1-N63                     1.00 (k[1])
    edges-B1-N64                     1.12 (q[1])
    edges-B1-N65                     1.08 (k[1])
    edges-B1-N256                    1.00 (q[1])
    edges-B1-N257                    0.99 (k[1])
    edges-B1-N320                    1.12 (q[1])
    edges-B2-N1                      1.47 (k[1])
    edges-B2-N7                      0.92 (states[1])
    edges-B2-N8                      1.09 (states[1])
    edges-B2-N9                      1.00 (k[1])
    edges-B2-N63                     1.22 (states[1])
    edges-B2-N64                     1.15 (q[1])
    edges-B2-N65                     1.11 (k[1])
    loop-B33-N1                      0.85 (q[1])
    loop-B5-N57                      1.05 (q[1])
    loop-B9-N33                      0.98 (states[1])
    rows-expanded-no-first-pos       1.00 (q[1])
    rows-expanded-with-first-pos     1.00 (q[1])
    rows-per_image-no-first-pos      1.06 (k[1])
    rows-per_image-with-first-pos    1.06 (k[1])
    rows-mixed-no-first-pos          1.15 (q[1])
    rows-mixed-with-first-pos        1.15 (q[1])
    ref-ratios                       1.53 (q[1])
    ref-premul                       1.52 (q[1])
    value-bias-mask                  0.97 (q[1])
    value-bias-nomask                1.09 (k[1])
    value-nobias-mask                1.01 (q[1])
    value-nobias-nomask              1.10 (q[1])
    mask-in-memory-S34000            1.05 (k[1])
    mask-in-memory-S32770            1.04 (k[1])
    mask-in-lds-S32750               1.09 (k[1])
    large-scores                     1.26 (states[1])
    depth-6                          1.28 (k[3])
"""
import copy
import ctypes
import warnings

import pytest
import torch

import decoder_layer_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

def _run(c):
    """(reference, float32 baseline, kernel results on the CPU, decoder on the device, inputs on the device)."""
    from egtr_amd import decoder_fused, ops
    dec, inp = R.build(c)
    ref = R.layer_f64(dec, inp)
    f32 = R.layer_f64(dec, inp, dtype=torch.float32)
    gdec = copy.deepcopy(dec).to(DEV).eval()
    ginp = R.to_device(inp, DEV)
    before = dict(ops.FALLBACKS)
    with torch.no_grad():
        states, q_all, k_all = decoder_fused.run(gdec, **ginp)
    torch.cuda.synchronize()
    assert decoder_fused.read_status(torch.device(DEV)) == 0
    assert ops.FALLBACKS == before, "the call left a fast path"
    B, N = c["B"], c["N"]
    assert tuple(states.shape) == (c["layers"], B, N, 256) and len(q_all) == len(k_all) == c["layers"]
    got = dict(states=states.cpu(), q=torch.stack([t.expand(B, N, 256) for t in q_all]).cpu(),
               k=torch.stack([t.expand(B, N, 256) for t in k_all]).cpu())
    return ref, f32, got


def _check(c, ref, f32, got):
    e32, err = R.errors(f32, ref), R.errors(got, ref)
    for b, i in R.outside_rows(c):   # all 128 samples outside: the cross-attention output is exactly the output bias
        assert bool((ref["cross_out"][-1, b, i] == 0).all())
    ratios = {key: err[key] / e32[key] for key in e32}
    worst = max(ratios, key=ratios.get)
    print(f"\n{c['name']}: kernel / e32 largest {ratios[worst]:.2f} at {worst}; "
          + " ".join(f"{o}[{l}] {err[(o, l)]:.2e}/{e32[(o, l)]:.2e}" for (o, l) in sorted(e32)))
    for key in sorted(e32):
        assert torch.isfinite(got[key[0]][key[1]]).all(), key
        assert err[key] <= R.FACTOR * e32[key], (c["name"], key, err[key], e32[key], ratios[key])


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["name"])
def test_decoder_layer_matches_the_float64_layer(c):
    _check(c, *_run(c))


def test_both_forms_of_the_reference_points_are_the_same_inputs():
    """The two "ref-" cases above are one set of points, once with the valid ratios applied by the kernel and once
    pre-multiplied: their float64 references agree to rounding of the float32 product."""
    a, b = (next(c for c in R.CASES if c["name"] == n) for n in ("ref-ratios", "ref-premul"))
    ia, ib = R.make_inputs(a), R.make_inputs(b)
    assert ia["valid_ratios"] is not None and ib["valid_ratios"] is None and tuple(ib["reference_input"].shape) == (2, 24, 4, 2)
    assert torch.equal(ia["reference_input"][:, :, None, :] * ia["valid_ratios"][:, None], ib["reference_input"])
    assert torch.equal(ia["values"], ib["values"])


def test_more_queries_than_the_kernel_holds_are_refused_without_a_launch(monkeypatch):
    from egtr_amd import _lib, decoder_fused, ops
    assert decoder_fused.MAX_QUERIES == 320
    dec = R.make_decoder(2, 1).to(DEV)
    monkeypatch.setattr(ops, "FALLBACKS", {})
    monkeypatch.setattr(ops, "STRICT_FAST_PATH", False)

    def z(*shape):
        return torch.zeros(*shape, device=DEV)

    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert decoder_fused.supported(dec, z(1, 320, 256), z(1, 320, 256), z(1, 320, 2), z(1, 256, 256), False)
        assert ops.FALLBACKS == {}
        assert not decoder_fused.supported(dec, z(1, 321, 256), z(1, 321, 256), z(1, 321, 2), z(1, 256, 256), False)
        assert ops.FALLBACKS == {"decoder_cluster": 1}
    a = decoder_fused.EgtrDecoderLayer()   # every pointer NULL: nothing could be launched from it
    a.batch, a.num_query, a.spatial_size, a.x_rows, a.pos_rows, a.qkv_rows, a.num_clusters = 1, 321, 256, 321, 321, 321, 41
    assert _lib.lib().egtr_decoder_layer_f32(None, ctypes.byref(a)) == -3   # EGTR_E_UNSUPPORTED
    a.num_query = a.x_rows = a.pos_rows = a.qkv_rows = 320
    a.num_clusters = 40
    assert _lib.lib().egtr_decoder_layer_f32(None, ctypes.byref(a)) == -1   # EGTR_E_ARG: served, but the pointers are missing


def test_inconsistent_cluster_and_row_counts_are_argument_errors(monkeypatch):
    """The arguments of a REAL launch (all buffers alive and large enough) with one count changed: refused with EGTR_E_ARG.
    The changed counts are smaller than the true ones, so every index they could produce stays inside the buffers."""
    from egtr_amd import _lib, decoder_fused
    c = R.case("refusals", 2, 24, seed=900)
    dec, inp = R.build(c)
    gdec, ginp = copy.deepcopy(dec).to(DEV).eval(), R.to_device(inp, DEV)
    seen = []
    launch = _lib.launch

    def recording(name, *args, **kw):
        if name == "egtr_decoder_layer_f32" and not seen:
            good = args[0]._obj
            assert good.num_clusters == 6 and good.qkv_rows == 48 and good.batch == 2 and good.num_query == 24
            fn = _lib.lib().egtr_decoder_layer_f32
            for field, value in (("num_clusters", 5), ("num_clusters", 0), ("qkv_rows", 25), ("qkv_rows", 0)):
                bad = decoder_fused.EgtrDecoderLayer.from_buffer_copy(good)
                setattr(bad, field, value)
                seen.append((field, value, fn(_lib._stream(), ctypes.byref(bad))))
        return launch(name, *args, **kw)

    monkeypatch.setattr(decoder_fused._lib, "launch", recording)
    with torch.no_grad():
        states, _, _ = decoder_fused.run(gdec, **ginp)
    torch.cuda.synchronize()
    assert seen == [("num_clusters", 5, -1), ("num_clusters", 0, -1), ("qkv_rows", 25, -1), ("qkv_rows", 0, -1)]
    assert decoder_fused.read_status(torch.device(DEV)) == 0
    ref = R.layer_f64(dec, inp)
    assert float((states.cpu().double() - ref["states"]).abs().max()) < 1e-4   # the launches that followed were whole
