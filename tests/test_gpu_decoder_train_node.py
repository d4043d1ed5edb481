"""GPU (-m gpu): the decoder layer's training node (egtr_amd.ops.DecoderLayerTrainFunction: 34 hand-wired gradients through
three LayerNorm backwards, nine skinny-linear backwards, the MSDA geometry backward and the self-attention backward, stitched
through addend / aliased-output epilogues) against the float64 layer of tests/decoder_train_restated.py -- torch ops under
autograd on the CPU, MSDA from F.grid_sample: none of the node's kernels.

Compared, every element of each: y3 and the retained scaled-q / k maps; the gradients of the states, the position rows (a
stride-0 batch expansion of the query table -- summed over the batch -- or rows per image), the reference points (through
``ref * valid_ratios``: summed over the levels), the value projection that is handed in, and all 24 parameters that receive one
(the layer's own value_proj receives none), with upstream gradients on y3 AND on both maps and the three dropout masks given.
Bound per tensor: max(plain, FACTOR x the float32 composition's error), plain = 4 u max|reference| (u = 2^-24: the float32
result is stored with up to u of relative rounding; the term only guards a yardstick that happens to be tiny), FACTOR = 4.  No
row or entry is left out: the cases keep away from the ReLU and pixel-boundary kinks by margins that
tests/test_decoder_train_cases_cpu.py measures.  Rows above 1024 per launch cannot keep away from them and are covered, exactly,
by tests/test_gpu_skinny_backward.py.

Measured on an MI355X over the ten cases, the largest kernel error / float32 composition's error per group (and the largest
error / bound): y3 1.22, q 0.83, k 0.94, grad_x 1.54, grad_pos 0.95, grad_ref 1.56, grad_value 1.73, parameters 2.22
(self_attn.k_proj.bias, B1-N9-ffn1024-p0) -- error / bound at most 0.56."""
import copy

import pytest
import torch

import decoder_train_restated as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _node(layer, inp, c, monkeypatch):
    """The layer module on the device in train mode, through its training node: the compared tensors by the reference's names."""
    from egtr_amd import ops
    monkeypatch.setattr(ops, "FALLBACKS", {})
    mod = copy.deepcopy(layer).to(DEV).train()
    mod.zero_grad(set_to_none=True)
    B, N = c["B"], c["N"]
    x, table, ref, value = (inp[n].to(DEV).clone().requires_grad_(True) for n in ("x", "pos", "ref", "value"))
    pos = table.unsqueeze(0).expand(B, -1, -1) if c["pos"] == "expanded" else table
    if c["pos"] == "expanded" and B > 1:
        assert pos.stride(0) == 0
    ref_in = ref * inp["ratios"].to(DEV)
    shapes, lsi = inp["shapes"].to(DEV), inp["lsi"].to(DEV)
    masks = inp["masks"].to(DEV) if inp["masks"] is not None else None
    assert ops.decoder_layer_train_supported(mod, x, pos, ref_in, value, None, False)
    outs = mod(x, position_embeddings=pos, reference_points=ref_in, spatial_shapes=shapes, level_start_index=lsi,
               encoder_hidden_states=value, encoder_attention_mask=None, output_attention_states=True,
               spatial_shapes_list=list(R.LEVELS), precomputed_value=value, dropout_masks=masks)
    y, qm, km = outs[0], outs[1], outs[2]
    assert type(y.grad_fn).__name__ == "DecoderLayerTrainFunctionBackward", type(y.grad_fn).__name__
    assert tuple(qm.shape) == (B, 8, N, 32)
    gy, gq, gk = (inp[n].to(DEV) for n in ("gy", "gq", "gk"))
    torch.autograd.backward([y, qm, km], [gy, gq.view(B, N, 8, 32).transpose(1, 2), gk.view(B, N, 8, 32).transpose(1, 2)])
    torch.cuda.synchronize()
    assert not ops.FALLBACKS, ops.FALLBACKS
    got = dict(y3=y.detach(), q=qm.detach().transpose(1, 2).reshape(B, N, 256), k=km.detach().transpose(1, 2).reshape(B, N, 256),
               grad_x=x.grad, grad_pos=table.grad, grad_ref=ref.grad, grad_value=value.grad)
    for n, q in mod.named_parameters():
        got[n] = q.grad
    return {n: (t.cpu() if t is not None else None) for n, t in got.items()}


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_decoder_layer_train_node_vs_float64_layer(name, monkeypatch):
    c = next(c for c in R.CASES if c["name"] == name)
    seed, layer, inp, r64, r32 = R.build(name)
    names = R.compared(r64)
    assert len(names) == 3 + 4 + 24
    got = _node(layer, inp, c, monkeypatch)
    for n in ("encoder_attn.value_proj.weight", "encoder_attn.value_proj.bias"):
        assert got[n] is None and r64[n] is None, n
    for n in names:
        assert got[n] is not None and got[n].shape == r64[n].shape and bool(torch.isfinite(got[n]).all()), n
    err, e32 = R.errors(got, r64, names), R.errors(r32, r64, names)
    failed = []
    for n in names:
        plain = 4 * U * float(r64[n].abs().max())
        bound = max(plain, R.FACTOR * e32[n])
        print(f"{name} seed {seed} {n}: kernel {err[n]:.3e} yardstick {e32[n]:.3e} ratio {err[n] / max(e32[n], 1e-300):.2f} "
              f"plain {plain:.3e} max|ref| {float(r64[n].abs().max()):.3e}")
        assert e32[n] > 0, n
        if err[n] > bound:
            failed.append((n, err[n], e32[n], plain))
    assert not failed, failed
