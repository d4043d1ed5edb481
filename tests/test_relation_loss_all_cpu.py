"""CPU: the un-sampled relation loss (evaluation mode / both ``rel_sample_*`` None; csrc/loss.hip rel_loss_all) -- what can be
checked without a GPU: the float64 restatement of tests/relation_loss_all_restated.py against the criterion's own tensor
composition (the last branch of ``loss_relations``: the reference's code path), the teeth of its three wrong neighbours on the
inputs the GPU tests use, the argument validation of the C entries, the ValueError of ``ops.relation_losses`` and
``DataParallelTrainer.validation_step`` / ``validation_epoch_end``."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import relation_loss_all_restated as RA


criterion = RA.criterion

COMPOSITION_CASES = [(n, False, False) for n in RA.case_names()] + [("n9r50", True, False), ("n9r50", False, True)]


@pytest.mark.parametrize("model_training", [False, True])
@pytest.mark.parametrize("name,nonbinary,sparse", COMPOSITION_CASES)
def test_restatement_equals_the_criterions_composition_in_float64(name, nonbinary, sparse, model_training):
    """Finite logits, float64 CPU tensors, every case (N = 1030 and the sparse and non-binary targets included): evaluation
    mode, and training mode with both sample counts None.  1e-12 relative on ``loss_rel``, and on its gradient relative to its
    largest element."""
    c = RA.case(name, "finite", nonbinary, sparse)
    crit = criterion(c["N"], c["R"], model_training)
    pr = c["pred_rel"].double().requires_grad_(True)
    pc = c["pred_conn"].double().requires_grad_(True)
    out = crit.loss_relations({"pred_rel": pr, "pred_connectivity": pc}, [{"rel": d.double()} for d in c["dense"]],
                              c["indices"], [x.double() for x in c["costs"]], 1.0)
    g_rel, = torch.autograd.grad(out["loss_rel"], pr)
    g_conn, = torch.autograd.grad(out["loss_connectivity"], pc)
    # the criterion holds its constant as an fp32 tensor; the restatement takes the same number
    l_rel, l_conn, r_rel, r_conn = RA.restate(c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"],
                                              nm_cost=float(crit.nonmatching_cost))
    assert out["loss_rel"].dtype == torch.float64
    assert abs(float(out["loss_rel"].detach()) - l_rel) <= 1e-12 * abs(l_rel)
    assert np.abs(g_rel.numpy() - r_rel).max() <= 1e-12 * np.abs(r_rel).max()
    # The composition builds its connectivity target as an fp32 tensor (egtr:789) whatever the logits are, and its connectivity
    # term comes back as fp32: it can agree with float64 to fp32 roundings only (4 of them: BCE, mean, and their gradient).
    assert out["loss_connectivity"].dtype == torch.float32
    tol = 4 * 2.0 ** -24
    assert abs(float(out["loss_connectivity"].detach()) - l_conn) <= tol * abs(l_conn)
    assert np.abs(g_conn.double().numpy() - r_conn).max() <= tol * np.abs(r_conn).max()


@pytest.mark.parametrize("nm_cost", [RA.NM_COST, RA.NM_HALF])
@pytest.mark.parametrize("name", RA.case_names())
def test_wrong_neighbours_have_teeth(name, nm_cost):
    """Dropped weights, an identity target map and unmatched queries weighted like matched ones move ``loss_rel`` by more than
    100 x the loss bar and a tenth of the gradient elements by more than 100 x the gradient bar -- on every case where the
    arithmetic lets them (RA.TEETH says where, and why not elsewhere).  Under the criterion's constant an unmatched query
    weighs 0 in fp32; with a non-matching cost of 0 (the second run of every case, on the GPU too) it weighs 1 / 2, and the
    map and the unmatched weight show in every case that has a relation and an unmatched query."""
    c = RA.case(name)
    args = (c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"], nm_cost)
    l_rel, _, g_rel, _ = RA.restate(*args)
    bar = RA.grad_bar(g_rel.size)
    for nb in RA.NEIGHBOURS:
        w_rel, _, wg_rel, _ = RA.restate(*args, neighbour=nb)
        moved_loss = abs(w_rel - l_rel) / abs(l_rel)
        moved_grad = float((np.abs(wg_rel - g_rel) > 100 * bar).mean())
        print(f"{name} nm_cost={nm_cost:.1f} {nb}: loss moves {moved_loss:.3e} relative, {moved_grad:.3f} of the gradient elements move")
        if nb in RA.TEETH[nm_cost][name]:
            assert moved_loss > 100 * RA.LOSS_BAR, (name, nb)
            assert moved_grad >= 0.1, (name, nb)
    for table in RA.TEETH.values():
        assert all(any(nb in t for t in table.values()) for nb in RA.NEIGHBOURS)
    if name == "n3r1":   # no relation: the three neighbours ARE the definition here
        assert all(RA.restate(*args, neighbour=nb)[0] == l_rel for nb in RA.NEIGHBOURS)


def test_sparse_targets_let_the_connectivity_see_a_wrong_map():
    """~20 triplets per image at R = 50: most pairs carry no relation, so a wrong target map moves ``loss_conn`` and its gradient
    (with 30 % of all elements set every pair is flagged, and the connectivity target is all ones)."""
    dense_all, c = RA.case("n9r50"), RA.case("n9r50", "finite", False, True)
    for b in (0, 2):
        assert bool((dense_all["dense"][b] != 0).any(-1).all())
        assert int(c["dense"][b].sum()) == RA.SPARSE_TRIPLETS and float((c["dense"][b] != 0).any(-1).float().mean()) < 0.3
    args = (c["pred_rel"], c["pred_conn"], c["dense"], c["indices"], c["costs"])
    _, l_conn, _, g_conn = RA.restate(*args)
    _, w_conn, _, wg_conn = RA.restate(*args, neighbour="identity_map")
    assert abs(w_conn - l_conn) > 100 * RA.LOSS_BAR * abs(l_conn)
    assert float((np.abs(wg_conn - g_conn) > 100 * RA.grad_bar(g_conn.size)).mean()) >= 0.1


def test_cases_hold_what_they_promise():
    for name in RA.case_names():
        B, N, R, matched = RA.CASES[name]
        fin, non = RA.case(name), RA.case(name, "nonfinite")
        x, xn = fin["pred_rel"].numpy(), non["pred_rel"].numpy()
        assert x.shape == (B, N, N, R) and np.isfinite(x).all()
        for v in RA.PLANTS:
            assert ((x == np.float32(v)) & (np.signbit(x) == np.signbit(np.float32(v)))).any(), (name, v)
        assert np.isposinf(xn).any() and np.isneginf(xn).any() and np.isnan(xn).any()
        for b, pred in enumerate(matched):
            assert [int(v) for v in fin["indices"][b][0]] == pred
            plant = list(RA.cost_plants(name, b)[:len(pred)])
            assert [float(v) for v in fin["costs"][b][:len(plant)]] == plant
            assert bool(fin["dense"][b].any()) != (b in RA.NO_RELATION.get(name, ()))
    pi, ti = RA.case("n5r4")["indices"][0]
    assert sorted(pi.tolist()) == list(range(5)) and pi.tolist() != sorted(pi.tolist()) and (pi != ti).any()
    assert bool(RA.case("n7r64")["dense"][0][..., 63].any())
    nb = RA.case("n9r50", "finite", True)["dense"][0]
    assert bool((nb == 0.5).any()) and bool((nb == 2.0).any())


# --------------------------------------------------------------------------------------------------------------- C entries
E_ARG, E_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from egtr_amd import _lib
    return _lib.lib()


def test_c_entries_exist_and_validate_without_a_gpu(lib):
    """The two symbols; NULL operands, non-positive sizes, ONE NULL gradient and an unknown target format are EGTR_E_ARG under
    every target format (0 dense, 1 words, 2 wide words), num_rel = 65 on packed words and 257 on wide words is
    EGTR_E_UNSUPPORTED -- all before any HIP call (the pointers below are host addresses no kernel ever sees)."""
    from egtr_amd import _lib
    for n in ("egtr_relation_loss_all_f32", "egtr_relation_loss_all_workspace_bytes"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # one entry, the target form an argument: no other un-sampled name in the table or in the header
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "egtr_hip.h")) as f:
        header = f.read()
    for names in ([n for n in _lib.SIGNATURES if n.startswith("egtr_relation_loss_all")],
                  re.findall(r"\b(egtr_relation_loss_all\w*)\s*\(", header)):
        assert sorted(set(names)) == ["egtr_relation_loss_all_f32", "egtr_relation_loss_all_workspace_bytes"]
    assert lib.egtr_abi_version() == 7 and _lib.ABI_VERSION == 7
    assert lib.egtr_status_string(E_UNSUPPORTED) and lib.egtr_status_string(E_ARG) != lib.egtr_status_string(E_UNSUPPORTED)
    assert lib.egtr_relation_loss_all_workspace_bytes(4, 200) >= 4 * 200 * 200 + 4 * 200 * 8
    assert lib.egtr_relation_loss_all_workspace_bytes(0, 200) == 0 and lib.egtr_relation_loss_all_workspace_bytes(4, -1) == 0
    raw = ctypes.create_string_buffer(64 + 16)
    p = (ctypes.addressof(raw) + 15) & ~15
    entry = lib.egtr_relation_loss_all_f32
    for fmt in (0, 1, 2):
        def call(ptrs=(p,) * 7, sizes=(2, 7, 5), out=(p, p, p, p), fmt=fmt):
            return entry(None, *ptrs[:3], fmt, *ptrs[3:], *sizes, 1.0, *out)
        assert call(ptrs=(None,) * 7, out=(None,) * 4) == E_ARG
        for i in range(7):                                        # each operand on its own
            assert call(ptrs=tuple(None if j == i else p for j in range(7))) == E_ARG, i
        assert call(out=(None, p, p, p)) == E_ARG                 # loss_out
        assert call(out=(p, p, p, None)) == E_ARG                 # workspace
        assert call(out=(p, None, p, p)) == E_ARG                 # one NULL gradient
        assert call(out=(p, p, None, p)) == E_ARG
        for sizes in ((0, 7, 5), (2, 0, 5), (2, 7, 0), (-1, 7, 5)):
            assert call(sizes=sizes) == E_ARG, sizes
        for bad in (-1, 3):                                       # an unknown format, every other operand valid
            assert call(fmt=bad) == E_ARG and call(fmt=bad, out=(p, None, None, p)) == E_ARG, bad
    for fmt, over in ((1, 65), (2, 257)):
        assert entry(None, p, p, p, fmt, p, p, p, p, 1, 6, over, 1.0, p, p, p, p) == E_UNSUPPORTED
        assert entry(None, p, p, p, fmt, p, p, p, p, 1, 6, over, 1.0, p, None, None, p) == E_UNSUPPORTED


def test_relation_losses_with_exactly_one_sample_count_raises():
    from egtr_amd import ops
    c = RA.case("n5r4")
    tg = [{"rel": d} for d in c["dense"]]
    for neg, nm in ((None, 80), (80, None)):
        with pytest.raises(ValueError, match="both sample counts or neither"):
            ops.relation_losses(c["pred_rel"], c["pred_conn"], tg, c["indices"], c["costs"], RA.NM_COST, neg, nm)
    assert ops.RELATION_LOSS_ALL is True and "RELATION_LOSS_ALL" not in " ".join(ops.ENV_ROUTE_SWITCHES)


def test_one_sided_none_and_cpu_tensors_keep_their_routes(monkeypatch):
    """The kernel route is for device fp32 logits with both counts set or both None: anything else never reaches
    ``ops.relation_losses``."""
    from egtr_amd import ops

    def never(*a, **k):
        raise AssertionError("ops.relation_losses must not be called")

    monkeypatch.setattr(ops, "relation_losses", never)
    c = RA.case("n5r4")
    outs = {"pred_rel": c["pred_rel"], "pred_connectivity": c["pred_conn"]}
    tg = [{"rel": d} for d in c["dense"]]
    for training in (False, True):
        crit = criterion(c["N"], c["R"], training)
        assert set(crit.loss_relations(outs, tg, c["indices"], c["costs"], 1.0)) == {"loss_rel", "loss_connectivity"}
    crit = criterion(c["N"], c["R"], True)
    crit.rel_sample_negatives = 80                # one-sided: the sampled tensor route
    crit.force_device_relations = True
    assert torch.isfinite(crit.loss_relations(outs, tg, c["indices"], c["costs"], 1.0)["loss_rel"])


# ----------------------------------------------------------------------------------------------------------------- trainer
class _Tiny(torch.nn.Module):
    """The forward contract of DetrForSceneGraphGeneration on a CPU model of one parameter: records the mode it ran in."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, -1.5]))
        self.frozen = torch.nn.BatchNorm1d(2)      # a submodule its owner keeps in evaluation mode while training
        self.seen = []
        self.fail = False

    def forward(self, pixel_values, pixel_mask, labels, **kw):
        self.seen.append((self.training, torch.is_grad_enabled()))
        import egtr_amd.deformable_detr as dd
        dd._STEP_MATCHER_STATUS.append(torch.zeros(1, dtype=torch.int32))     # what the device matcher does in a forward
        if self.fail:
            raise RuntimeError("forward failed")
        a, b = (self.w * pixel_values.mean()).unbind()
        return types.SimpleNamespace(loss=2.0 * a + 3.0 * b, loss_dict={"loss_rel": a, "loss_connectivity": b})


def _trainer():
    from egtr_amd.runtime import DataParallelTrainer
    model = _Tiny()
    return model, DataParallelTrainer(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), accumulate=1)


@pytest.mark.parametrize("was_training", [True, False])
def test_validation_step_on_a_cpu_model(was_training):
    model, tr = _trainer()
    model.train(was_training)
    model.frozen.eval()
    batch = {"pixel_values": torch.full((1, 3, 4, 4), 2.0), "pixel_mask": torch.ones(1, 4, 4, dtype=torch.long), "labels": []}
    import egtr_amd.deformable_detr as dd
    dd.DeformableDetrHungarianMatcher.take_step_statuses()
    window = torch.zeros(1, dtype=torch.int32)
    dd._STEP_MATCHER_STATUS.append(window)                                  # recorded by the accumulation window in flight
    loss, d = tr.validation_step(batch)
    assert len(dd._STEP_MATCHER_STATUS) == 1 and dd._STEP_MATCHER_STATUS[0] is window   # validation leaves none of its own
    assert model.seen == [(False, False)]                                   # evaluation mode, no autograd graph
    assert set(d) == {"loss_rel", "loss_connectivity", "loss"} and d["loss"] is loss
    assert float(loss) == 2.0 * 1.0 + 3.0 * -3.0 and float(d["loss_rel"]) == 1.0
    assert not loss.requires_grad and not any(v.requires_grad for v in d.values())
    assert all(p.grad is None for p in model.parameters())
    assert model.training is was_training and tr.model is model and model.frozen.training is False
    model.fail = True
    with pytest.raises(RuntimeError, match="forward failed"):
        tr.validation_step(batch)
    assert model.training is was_training and tr.model is model
    assert dd.DeformableDetrHungarianMatcher.take_step_statuses() == [window]
    model.fail = False
    if was_training:                                                        # the training step still works afterwards
        tr.training_step(batch)
        assert model.seen[-1] == (True, True)


def test_validation_epoch_end_is_the_mean_per_key():
    from egtr_amd.runtime import DataParallelTrainer
    steps = [(torch.tensor(1.0), {"loss_rel": torch.tensor(0.25), "loss": torch.tensor(1.0)}),
             (torch.tensor(2.0), {"loss_rel": torch.tensor(0.75), "loss": torch.tensor(2.0)}),
             (torch.tensor(6.0), {"loss_rel": torch.tensor(2.0), "loss": torch.tensor(6.0)})]
    want = {"validation_loss_rel": 1.0, "validation_loss": 3.0}
    assert DataParallelTrainer.validation_epoch_end(steps) == want
    assert DataParallelTrainer.validation_epoch_end([d for _, d in steps]) == want      # the reference returns the dicts alone
    assert all(type(v) is float for v in want.values()) and DataParallelTrainer.validation_epoch_end([]) == {}
