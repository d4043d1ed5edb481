"""Golden vectors for a predicate vocabulary beyond 64 classes, produced by RUNNING THE REFERENCE (model/egtr.py:366-416 relation
head, :509-512 logit adjustment, :754-923 relation losses -- all generic in the number of predicates) on seeded weights and inputs:

    python tests/golden/make_golden_wide.py      -> tests/golden/sgg_small_wide.npz

num_rel_labels = 100, num_labels = 12, num_queries = 24, Le = 2, Ld = 3, 2 images (one padded) of 96 x 128, use_freq_bias = True,
auxiliary losses on.  Stores the eval-mode outputs (pre-sigmoid relation / connectivity logits; with logit_adjustment = True the
adjusted pred_rel of every second subject), the eval-mode (un-sampled) and train-mode loss dicts and every gradient norm."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference under the shims of _ref_import, installs the stub backbone)
import weights as W  # noqa: E402


def main():
    model, cfg, cfg_dict, shapes = MG.build_ref_model(dict(num_rel_labels=100, auxiliary_loss=True), seed=101)
    model.eval()
    rng = W.rng_inputs(102)
    B, H, Wd = 2, 96, 128
    pv = torch.from_numpy(rng.standard_normal((B, 3, H, Wd))).float()
    pm = torch.ones(B, H, Wd, dtype=torch.long)
    pm[1, 80:, :] = 0
    pm[1, :, 104:] = 0
    pv[1] = pv[1] * pm[1][None].float()
    targets = W.make_targets(103, B, cfg.num_queries, cfg.num_labels, cfg.num_rel_labels)
    res = dict(cfg=json.dumps(cfg_dict), shapes=json.dumps(shapes), seed=101, input_seed=102, target_seed=103, H=H, W=Wd,
               valid1=np.array([80, 104]))
    with torch.no_grad():
        out, cap, _ = MG.run_ref(model, pv, pm)
        out_e, _, _ = MG.run_ref(model, pv, pm, labels=targets)
        model.config.logit_adjustment = True
        out_la, _, _ = MG.run_ref(model, pv, pm)
        model.config.logit_adjustment = False
    # rel_mlp is the MLP's output BEFORE the frequency bias (egtr:402-413); pred_rel = sigmoid(rel_mlp + bias)
    res.update(logits=MG.np_(out.logits), pred_boxes=MG.np_(out.pred_boxes), rel_mlp=MG.np_(cap["rel_mlp"]),
               conn_logits=MG.np_(cap["conn"]), pred_rel_last=MG.np_(out.pred_rel[..., -1]),
               pred_rel_adjusted=MG.np_(out_la.pred_rel[:, ::2]))
    res["eval_loss"] = MG.np_(out_e.loss)
    res["eval_loss_dict"] = json.dumps({k: float(v) for k, v in out_e.loss_dict.items()})
    model.train()
    model.zero_grad()
    out_t, _, _ = MG.run_ref(model, pv, pm, labels=targets)
    out_t.loss.backward()
    res["train_loss"] = MG.np_(out_t.loss)
    res["train_loss_dict"] = json.dumps({k: float(v) for k, v in out_t.loss_dict.items()})
    res["grad_norms"] = json.dumps({n: float(p.grad.norm()) for n, p in model.named_parameters() if p.grad is not None})
    path = os.path.join(HERE, "sgg_small_wide.npz")
    np.savez_compressed(path, **res)
    print("sgg_small_wide.npz", os.path.getsize(path), float(out_t.loss), float(out_e.loss), tuple(out.pred_rel.shape))


if __name__ == "__main__":
    main()
