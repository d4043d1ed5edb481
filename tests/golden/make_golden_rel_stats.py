"""Golden vectors of the relation statistics and the zero-shot recall, produced by RUNNING THE REFERENCE:

  * data.visual_genome.vg_get_statistics and data.open_image.oi_get_statistics are imported from the reference tree and fed
    duck-typed stand-ins for their ``train_data`` (rel_stats_inputs.train_split): ``.coco.cats`` / ``.coco.getAnnIds`` /
    ``.coco.loadAnns`` / ``.ids`` / ``.rel`` / ``.rel_categories`` with ONE-based ``category_id`` and predicates (the function
    shifts the predicate by one), and ``.targets`` / ``.ind_to_classes`` / ``.rel_categories``.  An image without a relation hands
    the functions an empty [0, 3] array: both index a 2-d array.  torchvision (absent here) is only the base class of the
    dataset classes in that module, which are not used; an inert stand-in module lets the import pass.
  * zero-shot recall: the reference's BasicSceneGraphEvaluator (sgdet, both multiple_preds settings; the real sg_eval
    module with the reference's Cython bbox module, as in make_golden_sgg_eval.py) is called per test image with
    ``gt_relations`` FILTERED to the zero-shot rows -- the rows whose (class, class, predicate) count is zero in the
    reference's own fg_matrix.  Its per-image recalls are the reference values of zR@k.  The same with the first 10
    candidates only (``k10_``: fewer candidates than the smallest k).

    make -C oracle ref && python tests/golden/make_golden_rel_stats.py      -> tests/golden/rel_stats.npz

The conditions asserted before writing make the numbers mean something; if a seed misses one, change the seed
(rel_stats_inputs.SEED), not the conditions."""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import rel_stats_inputs as RI  # noqa: E402

KS = (20, 50, 100)


def import_reference():
    from oracle import ref_bbox
    bbox = ref_bbox.load()
    assert bbox is not None, "run `make -C oracle ref` first"
    import _ref_import
    _ref_import.load_reference()
    sys.modules["lib.fpn.box_intersections_cpu.bbox"] = bbox
    import lib.evaluation.sg_eval as sg_eval
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.datasets = types.ModuleType("torchvision.datasets")
        tv.datasets.CocoDetection = object
        sys.modules["torchvision"], sys.modules["torchvision.datasets"] = tv, tv.datasets
    from data.open_image import oi_get_statistics
    from data.visual_genome import vg_get_statistics
    return sg_eval, vg_get_statistics, oi_get_statistics


class _Coco:
    def __init__(self, split):
        self.cats = {c + 1: {"id": c + 1} for c in range(RI.C)}
        self._anns = {i: [{"category_id": int(c) + 1} for c in classes] for i, (classes, _) in enumerate(split)}

    def getAnnIds(self, image_id):
        return image_id

    def loadAnns(self, image_id):
        return self._anns[image_id]


class VGTrainData:
    """What vg_get_statistics reads of a VGDataset."""

    def __init__(self, split):
        self.coco = _Coco(split)
        self.ids = list(range(len(split)))
        self.rel_categories = [f"p{p}" for p in range(RI.R)]      # 'no_relation' already removed (visual_genome.py:53)
        self.rel = {str(i): (rows + np.array([0, 0, 1])).tolist() if len(rows) else np.zeros((0, 3))
                    for i, (_, rows) in enumerate(split)}

    def __len__(self):
        return len(self.ids)


class OITrainData:
    """What oi_get_statistics reads of an OIDataset."""

    def __init__(self, split):
        self.ind_to_classes = [f"c{c}" for c in range(RI.C)]
        self.rel_categories = [f"p{p}" for p in range(RI.R)]
        self.targets = [{"det_labels": classes.tolist(), "rel": rows.tolist() if len(rows) else np.zeros((0, 3), np.int64)}
                        for classes, rows in split]


def zero_shot_recalls(sg_eval, fg, cands, targets, gt_boxes, mode, top=None):
    """Per image with a zero-shot GT triplet: the reference evaluator's recalls on the zero-shot rows -> [n, nk]; and the
    evaluator's recalls on ALL rows -> [B, nk]."""
    multiple = mode == "m"
    ev_z = sg_eval.BasicSceneGraphEvaluator.all_modes(multiple_preds=multiple)["sgdet"]
    ev_a = sg_eval.BasicSceneGraphEvaluator.all_modes(multiple_preds=multiple)["sgdet"]
    for c, t, gb in zip(cands, targets, gt_boxes):
        rels, cls = t["rel_triplets"].numpy(), t["class_labels"].numpy()
        zs = fg[cls[rels[:, 0]], cls[rels[:, 1]], rels[:, 2]] == 0
        pred = {"pred_boxes": c["pred_boxes"].numpy(), "pred_classes": c["pred_classes"].numpy(),
                "obj_scores": np.ones(RI.N), "pred_rel_inds": c[f"{mode}_inds"].numpy()[:top],
                "rel_scores": c[f"{mode}_scores"].numpy()[:top]}
        ev_a.evaluate_scene_graph_entry({"gt_relations": rels, "gt_boxes": gb, "gt_classes": cls}, pred)
        if zs.any():
            ev_z.evaluate_scene_graph_entry({"gt_relations": rels[zs], "gt_boxes": gb, "gt_classes": cls}, pred)
    with contextlib.redirect_stdout(io.StringIO()):
        stats = ev_z.print_stats()
    rec = lambda ev: np.array([ev.result_dict["sgdet_recall"][k] for k in KS]).T      # noqa: E731
    return rec(ev_z), rec(ev_a), np.array([stats[f"R@{k}"] for k in KS])


def main():
    sg_eval, vg_stats, oi_stats = import_reference()
    split = RI.train_split()
    with contextlib.redirect_stderr(io.StringIO()):      # tqdm
        fg_vg = vg_stats(VGTrainData(split))
        fg_oi = oi_stats(OITrainData(split))
    assert fg_vg.dtype == fg_oi.dtype == np.int64 and fg_vg.shape == (RI.C + 1, RI.C + 1, RI.R)
    assert np.array_equal(fg_vg, fg_oi) and np.array_equal(fg_vg, RI.count(split))
    assert fg_vg.sum() == sum(len(r) for _, r in split)
    assert any(len(np.unique(r, axis=0)) < len(r) for _, r in split), "no duplicated row"
    assert any(len(c) and not len(r) for c, r in split) and any(not len(c) for c, _ in split)

    cands, targets, gt_boxes = RI.test_split()
    res = {"fg_vg": fg_vg, "fg_oi": fg_oi, "n_zero_shot": []}
    for t, gb in zip(targets, gt_boxes):
        # the pixel boxes are what rescale_bboxes gives for the stored normalised boxes, exactly
        cx, cy, w, h = t["boxes"].numpy().T
        back = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], 1) * np.array(
            [RI.W_IMG, RI.H_IMG, RI.W_IMG, RI.H_IMG], np.float32)
        assert back.dtype == np.float32 and np.array_equal(back, gb)
        rels, cls = t["rel_triplets"].numpy(), t["class_labels"].numpy()
        assert len(rels) and len(np.unique(rels, axis=0)) == len(rels)
        res["n_zero_shot"].append(int((fg_vg[cls[rels[:, 0]], cls[rels[:, 1]], rels[:, 2]] == 0).sum()))
    nz = np.array(res["n_zero_shot"])
    n_rel = np.array([len(t["rel_triplets"]) for t in targets])
    assert (nz > 0).sum() >= 3 and (nz == 0).sum() >= 3, nz
    assert ((nz > 0) & (nz < n_rel)).any(), "no image mixes zero-shot and seen triplets"
    for mode in ("m", "s"):
        zs, full, stats = zero_shot_recalls(sg_eval, fg_vg, cands, targets, gt_boxes, mode)
        zs10, _, stats10 = zero_shot_recalls(sg_eval, fg_vg, cands, targets, gt_boxes, mode, top=10)
        assert zs.shape == ((nz > 0).sum(), len(KS))
        hits = zs * nz[nz > 0][:, None]                    # zero-shot triplets hit below k, per image
        assert hits[:, 0].sum() > 0, "no zero-shot triplet hit below 20"
        assert (hits[:, 1] - hits[:, 0]).sum() > 0, "none hit only between 20 and 50"
        assert (nz[nz > 0] - hits[:, 2]).sum() > 0, "none missed"
        assert 0 < stats[2] < 1, stats
        assert stats[0] != full[:, 0].mean(), "zR@20 == R@20"
        res[f"{mode}_zs_recall"], res[f"{mode}_recall"], res[f"{mode}_zs_stats"] = zs, full, stats
        res[f"k10_{mode}_zs_recall"], res[f"k10_{mode}_zs_stats"] = zs10, stats10
        print(mode, "zR@k", stats, "R@k", full.mean(0), "zR@k with 10 candidates", stats10)
    res["n_zero_shot"] = nz
    np.savez_compressed(os.path.join(HERE, "rel_stats.npz"), seed=RI.SEED, **res)
    print("zero-shot GT triplets per test image", nz, "of", n_rel)
    print("fg_matrix: sum", fg_vg.sum(), "non-empty cells", (fg_vg > 0).sum(), "of", fg_vg[:RI.C, :RI.C].size)


if __name__ == "__main__":
    main()
