"""CPU: the ragged ground-truth packers of the evaluators (egtr_amd.evaluation._common.pack_relation_gt for
csrc/sgg_eval.hip and oi_eval.hip, egtr_amd.evaluation.coco.pack_coco_gt for csrc/coco_eval.hip) write the byte layout
the kernels read.  Every expected value is written out by hand from the documented layouts."""
import torch

from egtr_amd.evaluation._common import pack_relation_gt, relation_layout, relation_views
from egtr_amd.evaluation.coco import coco_layout, pack_coco_gt

FILL = 0xAB     # what the buffer holds before packing: bytes past the layout must keep it


def relation_batch():
    """Three images as ``gt_entry`` gives them: no GT relations, no boxes at all, two boxes with two relations."""
    return [{"gt_relations": torch.zeros(0, 3, dtype=torch.int64),
             "gt_boxes": torch.tensor([[10., 11., 12., 13.], [14., 15., 16., 17.], [18., 19., 20., 21.]]),
             "gt_classes": torch.tensor([1, 2, 3])},
            {"gt_relations": torch.zeros(0, 3, dtype=torch.int64), "gt_boxes": torch.zeros(0, 4),
             "gt_classes": torch.zeros(0, dtype=torch.int64)},
            {"gt_relations": torch.tensor([[0, 1, 3], [1, 0, 2]]),
             "gt_boxes": torch.tensor([[1., 2., 3., 4.], [5.5, 6.5, 7.5, 8.5]]), "gt_classes": torch.tensor([5, 7])}]


def test_relation_packer_writes_the_documented_bytes():
    gts = relation_batch()
    lay = relation_layout(gts)
    # B = 3, T = 2, G = 5: int64 [rel_off 4 | box_off 4 | rels 6 | classes 5] = 19 words = 152 bytes, then 20 float32
    assert tuple(lay) == (2, 5, 4, 8, 14, 152, 232)
    buf = torch.full((256,), FILL, dtype=torch.uint8)
    pack_relation_gt(gts, lay, buf)
    assert buf[:152].view(torch.int64).tolist() == [0, 0, 0, 2,            # rel_off
                                                    0, 3, 3, 5,            # box_off
                                                    0, 1, 3, 1, 0, 2,      # rels (s, o, p) x 2
                                                    1, 2, 3, 5, 7]         # classes
    assert buf[152:232].view(torch.float32).tolist() == [10., 11., 12., 13., 14., 15., 16., 17., 18., 19., 20., 21.,
                                                         1., 2., 3., 4., 5.5, 6.5, 7.5, 8.5]
    assert buf[232:].tolist() == [FILL] * 24
    gt = relation_views(buf[:232], lay)
    assert gt.rel_off.tolist() == [0, 0, 0, 2] and gt.box_off.tolist() == [0, 3, 3, 5]
    assert gt.rels.tolist() == [0, 1, 3, 1, 0, 2] and gt.classes.tolist() == [1, 2, 3, 5, 7]
    assert gt.boxes.dtype == torch.float32 and gt.boxes.numel() == 20 and gt.boxes[16:].tolist() == [5.5, 6.5, 7.5, 8.5]
    base = buf.data_ptr()
    assert [gt.rel_off.data_ptr() - base, gt.box_off.data_ptr() - base, gt.rels.data_ptr() - base,
            gt.classes.data_ptr() - base, gt.boxes.data_ptr() - base] == [0, 32, 64, 112, 152]


def test_relation_packer_without_relations_or_boxes():
    gts = relation_batch()[:2]            # T = 0: no rels section; the kernels get a null pointer for it
    lay = relation_layout(gts)
    assert tuple(lay) == (0, 3, 3, 6, 6, 72, 120)
    buf = torch.full((120,), FILL, dtype=torch.uint8)
    pack_relation_gt(gts, lay, buf)
    assert buf[:72].view(torch.int64).tolist() == [0, 0, 0, 0, 3, 3, 1, 2, 3]
    gt = relation_views(buf, lay)
    assert gt.rels is None and gt.classes.tolist() == [1, 2, 3] and gt.boxes.numel() == 12
    gts = relation_batch()[1:2]           # G = 0 as well: offsets only
    lay = relation_layout(gts)
    assert tuple(lay) == (0, 0, 2, 4, 4, 32, 32)
    buf = torch.full((32,), FILL, dtype=torch.uint8)
    pack_relation_gt(gts, lay, buf)
    assert buf.view(torch.int64).tolist() == [0, 0, 0, 0]
    gt = relation_views(buf, lay)
    assert gt.rels is None and gt.boxes is None and gt.classes is None
    assert gt.rel_off.tolist() == [0, 0] and gt.box_off.tolist() == [0, 0]


def coco_batch():
    """Three images as ``_coco_gt`` gives them: two GTs (one a crowd), none, one."""
    def gt(boxes, area, crowd, labels):
        return {"boxes": torch.tensor(boxes, dtype=torch.float64).reshape(-1, 4),
                "area": torch.tensor(area, dtype=torch.float64), "iscrowd": torch.tensor(crowd, dtype=torch.uint8),
                "labels": torch.tensor(labels, dtype=torch.int64)}
    return [gt([[1., 2., 3., 4.], [5., 6., 7., 8.]], [12., 56.], [0, 1], [4, 9]), gt([], [], [], []),
            gt([[0.5, 1.5, 2.5, 3.5]], [8.75], [0], [2])]


def test_coco_packer_writes_the_documented_bytes():
    g = coco_batch()
    lay = coco_layout(g)
    # B = 3, G = 3: int64 [offsets 4 | labels 3] = 56 bytes, fp64 [boxes 12 | area 3] = 120 bytes, then 3 crowd bytes
    assert tuple(lay) == (3, 4, 56, 176, 179)
    buf = torch.full((192,), FILL, dtype=torch.uint8)
    pack_coco_gt(g, lay, buf)
    assert buf[:56].view(torch.int64).tolist() == [0, 2, 2, 3,      # offsets
                                                   4, 9, 2]         # labels
    assert buf[56:176].view(torch.float64).tolist() == [1., 2., 3., 4., 5., 6., 7., 8., 0.5, 1.5, 2.5, 3.5,   # boxes xywh
                                                        12., 56., 8.75]                                       # area
    assert buf[176:179].tolist() == [0, 1, 0]
    assert buf[179:].tolist() == [FILL] * 13


def test_coco_packer_without_boxes():
    g = coco_batch()[1:2]
    lay = coco_layout(g)
    assert tuple(lay) == (0, 2, 16, 16, 16)
    buf = torch.full((16,), FILL, dtype=torch.uint8)
    pack_coco_gt(g, lay, buf)
    assert buf.view(torch.int64).tolist() == [0, 0]
