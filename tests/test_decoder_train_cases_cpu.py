"""CPU: the cases of tests/test_gpu_decoder_train_node.py (tests/decoder_train_restated.py) keep away from the layer's kinks by
the stated margins, the margins are 16 x the float32 deviation measured here, and the cases resolve every listed defect of the
gradient wiring."""
import pytest
import torch

import decoder_train_restated as R

NAMES = [c["name"] for c in R.CASES]
U = 2.0 ** -24


def _bounds(r64, r32, names):
    """Per tensor: the GPU test's bound max(plain, FACTOR x float32 composition's error)."""
    e32 = R.errors(r32, r64, names)
    return {n: max(4 * U * float(r64[n].abs().max()), R.FACTOR * e32[n]) for n in names}


@pytest.mark.parametrize("name", NAMES)
def test_case_keeps_away_from_the_kinks(name):
    c = next(c for c in R.CASES if c["name"] == name)
    seed, layer, inp, r64, r32 = R.build(name)
    d_relu, d_px = R.kink_distances(r64)
    print(f"{name}: seed {seed} (base {c['base_seed']}), min |fc1 pre-activation| {d_relu:.3e}, min pixel-boundary distance "
          f"{d_px:.3e}")
    assert c["base_seed"] <= seed < c["base_seed"] + R.MAX_SEEDS
    assert d_relu >= R.DELTA_RELU and d_px >= R.DELTA_PX
    assert R.same_branches(r32, r64)
    assert tuple(r64["pre"].shape) == (c["B"], c["N"], c["ffn"]) and r64["px"].numel() == c["B"] * c["N"] * 8 * 16 * 2
    # what is compared: forward, four state gradients, 24 parameters; the layer's own value projection receives nothing
    names = R.compared(r64)
    assert len(names) == 3 + 4 + 24 and not any("value_proj" in n for n in names)
    assert r64["encoder_attn.value_proj.weight"] is None and r64["encoder_attn.value_proj.bias"] is None
    assert tuple(r64["grad_pos"].shape) == ((c["N"], 256) if c["pos"] == "expanded" else (c["B"], c["N"], 256))
    assert tuple(r64["grad_ref"].shape) == (c["B"], c["N"], 1, 2) and tuple(r64["grad_value"].shape) == (c["B"], R.S, 256)
    e32 = R.errors(r32, r64, names)
    assert all(e > 0 for e in e32.values()), e32                     # the yardstick of every tensor
    # about half of the ReLU inputs on either side, samples inside and outside the levels
    frac = float((r64["pre"] > 0).double().mean())
    assert 0.2 < frac < 0.8
    wh = torch.tensor([[w, h] for h, w in R.LEVELS], dtype=torch.float64)[None, None, None, :, None, :]
    inside = ((r64["px"] > -1) & (r64["px"] < wh)).all(-1)
    assert 0.3 < float(inside.double().mean()) <= 1.0


def test_margins_are_sixteen_times_the_measured_float32_deviation():
    dev_relu = dev_px = 0.0
    for name in NAMES:
        _, _, _, r64, r32 = R.build(name)
        a, b = R.deviations(r32, r64)
        dev_relu, dev_px = max(dev_relu, a), max(dev_px, b)
    print(f"largest float32 deviation over the cases: fc1 pre-activation {dev_relu:.3e}, pixel coordinate {dev_px:.3e}; "
          f"delta_relu = 16 x = {R.MARGIN_FACTOR * dev_relu:.3e} (margin in use {R.DELTA_RELU:.1e}), "
          f"delta_px = 16 x = {R.MARGIN_FACTOR * dev_px:.3e} (margin in use {R.DELTA_PX:.1e})")
    print("chosen seeds: " + ", ".join(f"{n}: {R.build(n)[0]}" for n in NAMES))
    assert dev_relu > 0 and dev_px > 0
    assert R.MARGIN_FACTOR * dev_relu <= R.DELTA_RELU and R.MARGIN_FACTOR * dev_px <= R.DELTA_PX


@pytest.mark.parametrize("defect", [d[0] for d in R.DEFECTS])
def test_a_case_resolves_the_defect(defect):
    """The defective wiring leaves the GPU test's bound of some compared tensor by at least 10 x, at a case that is named."""
    shows = dict(R.DEFECTS)[defect]
    tried = []
    for c in sorted((c for c in R.CASES if shows(c)), key=lambda c: c["B"] * c["N"] * c["ffn"]):
        _, layer, inp, r64, r32 = R.build(c["name"])
        names = R.compared(r64)
        bad = R.compose(layer, inp, torch.float64, edit=defect)
        for n in R.FORWARD:
            assert float((bad[n] - r64[n]).abs().max()) <= 1e-12 * max(1.0, float(r64[n].abs().max())), (defect, n)
        err, bound = R.errors(bad, r64, names), _bounds(r64, r32, names)
        worst = max(names, key=lambda n: err[n] / bound[n])
        tried.append(c["name"])
        if err[worst] >= 10 * bound[worst]:
            print(f"defect '{defect}': resolved by case {c['name']} in {worst}: {err[worst]:.3e} against a bound of "
                  f"{bound[worst]:.3e}")
            return
    assert False, f"defect '{defect}': no case among {tried} shows it 10 x above the bound"


def test_restatement_states_the_module(cpu_kernels, monkeypatch):
    """The float32 composition against the layer module itself on the CPU (its generic per-operation route, MSDA and
    self-attention from the oracle stand-ins), dropout off: forward and gradients agree to float32 rounding."""
    from egtr_amd import ops
    name = next(c["name"] for c in R.CASES if c["p"] == 0 and c["pos"] == "expanded" and c["B"] >= 2)
    _, layer, inp, r64, r32 = R.build(name)
    monkeypatch.setattr(ops, "FALLBACKS", {})
    mod = __import__("copy").deepcopy(layer)
    mod.zero_grad(set_to_none=True)
    x = inp["x"].clone().requires_grad_(True)
    table = inp["pos"].clone().requires_grad_(True)
    ref = inp["ref"].clone().requires_grad_(True)
    value = inp["value"].clone().requires_grad_(True)
    B, N = x.shape[:2]
    outs = mod(x, position_embeddings=table.unsqueeze(0).expand(B, -1, -1), reference_points=ref * inp["ratios"],
               spatial_shapes=inp["shapes"], level_start_index=inp["lsi"], encoder_hidden_states=value,
               encoder_attention_mask=None, output_attention_states=True, spatial_shapes_list=list(R.LEVELS),
               precomputed_value=value, dropout_masks=None)
    y, qm, km = outs[0], outs[1], outs[2]
    torch.autograd.backward([y, qm, km], [inp["gy"], inp["gq"].view(B, N, 8, 32).transpose(1, 2),
                                          inp["gk"].view(B, N, 8, 32).transpose(1, 2)])
    got = dict(y3=y.detach(), q=qm.detach().transpose(1, 2).reshape(B, N, 256), k=km.detach().transpose(1, 2).reshape(B, N, 256),
               grad_x=x.grad, grad_pos=table.grad, grad_ref=ref.grad, grad_value=value.grad)
    for n, q in mod.named_parameters():
        got[n] = q.grad
    for n in R.compared(r64):
        err = float((got[n].double() - r64[n]).abs().max())
        assert err <= 2e-4 * max(1.0, float(r64[n].abs().max())), (n, err)
