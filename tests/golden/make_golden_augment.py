"""Writes tests/golden/augment.npz: what the reference's training augmentation makes of seeded images and boxes.

The chain is built from the reference's own model/transform.py classes (Compose / RandomHorizontalFlip / RandomSelect /
RandomResize / RandomSizeCrop), loaded from its file under a stub `torchvision` defined here (torchvision is not
installed): PIL-backed functional.crop / hflip / resize, transforms.RandomCrop.get_params and ops.boxes.box_area restated
from torchvision 0.13 (not confirmed against an install).  The stub logs every flip, resize and crop, so the fixture
records what the chain did and not only what came out.  Runs only where the reference tree exists; contains none of it.

Two parts:
  small, with pixels      scaled-down constants, a dozen images, both variants (crop / no crop): raw pixels, seeds, the
                          logged parameters, the next draw of `random` and torch after the chain, the output targets and
                          pixel_values / pixel_mask after the restated 4.18 rescale, normalise and pad
  full, without pixels    the reference's constants on a few hundred (h, w) with boxes: seeds, logged parameters, output
                          targets, and the sha256 of the final uint8 image for a handful

    python tests/golden/make_golden_augment.py"""
import hashlib
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_import import REF_ROOT  # noqa: E402  (where the read-only reference tree lives; nothing else is used)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SMALL = dict(scales=[24, 28, 32, 36, 40], mid_sizes=[20, 25, 30], crop_range=(19, 30), max_size=64)
FULL = dict(scales=[480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800], mid_sizes=[400, 500, 600],
            crop_range=(384, 600), max_size=1333)
SMALL_SHAPES = [(23, 31), (40, 17), (20, 20), (25, 64), (30, 22), (13, 47), (37, 37), (50, 20), (21, 90), (33, 25),
                (28, 36), (60, 45)]
N_FULL, N_SHA = 300, 6
LOG = []


def install_stub_torchvision():
    tv = types.ModuleType("torchvision")
    tv.__version__ = "0.13.0"
    tr = types.ModuleType("torchvision.transforms")
    fn = types.ModuleType("torchvision.transforms.functional")
    ops = types.ModuleType("torchvision.ops")
    boxes = types.ModuleType("torchvision.ops.boxes")

    def crop(img, top, left, height, width):
        LOG.append(("crop", top, left, height, width))
        return img.crop((left, top, left + width, top + height))

    def hflip(img):
        LOG.append(("hflip",))
        return img.transpose(Image.FLIP_LEFT_RIGHT)

    def resize(img, size):
        LOG.append(("resize", size[0], size[1]))
        return img.resize(tuple(size[::-1]), Image.BILINEAR)

    class RandomCrop:
        @staticmethod
        def get_params(img, output_size):
            w, h = img.size
            th, tw = output_size
            if h + 1 < th or w + 1 < tw:
                raise ValueError("Required crop size is larger then input image size")
            if w == tw and h == th:
                return 0, 0, h, w
            i = torch.randint(0, h - th + 1, size=(1,)).item()
            j = torch.randint(0, w - tw + 1, size=(1,)).item()
            return i, j, th, tw

    def box_area(b):
        return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])

    fn.crop, fn.hflip, fn.resize = crop, hflip, resize
    tr.RandomCrop, tr.functional = RandomCrop, fn
    boxes.box_area, ops.boxes = box_area, boxes
    tv.transforms, tv.ops = tr, ops
    for m in (tv, tr, fn, ops, boxes):
        sys.modules[m.__name__] = m


def load_reference_transform():
    install_stub_torchvision()
    if REF_ROOT not in sys.path:
        sys.path.insert(0, REF_ROOT)
    spec = importlib.util.spec_from_file_location("_reference_transform", os.path.join(REF_ROOT, "model", "transform.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_chain(T, crop, scales, mid_sizes, crop_range, max_size):
    second = [T.RandomResize(list(mid_sizes))]
    if crop:
        second.append(T.RandomSizeCrop(*crop_range))
    second.append(T.RandomResize(list(scales), max_size=max_size))
    return T.Compose([T.RandomHorizontalFlip(),
                      T.RandomSelect(T.RandomResize(list(scales), max_size=max_size), T.Compose(second))])


def make_boxes(rng, h, w, n):
    """Boxes of every size, some hugging a border so that a crop drops them."""
    x0 = rng.uniform(0, w - 1, n)
    y0 = rng.uniform(0, h - 1, n)
    x1 = np.minimum(x0 + rng.uniform(0.5, w / 2, n), w)
    y1 = np.minimum(y0 + rng.uniform(0.5, h / 2, n), h)
    b = np.stack([x0, y0, x1, y1], 1).astype(np.float32)
    b[0] = (0, 0, max(1.0, w * 0.05), max(1.0, h * 0.05))            # top-left corner
    b[1] = (w * 0.95, h * 0.95, w, h)                                  # bottom-right corner
    return b


def run_case(chain, img, boxes, seed):
    """One image through the chain under one seed: the logged parameters, the output image and targets, and the next
    draw of both generators."""
    n = len(boxes)
    target = {"boxes": torch.from_numpy(boxes.copy()), "class_labels": torch.arange(n) % 7,
              "area": torch.from_numpy((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])),
              "iscrowd": (torch.arange(n) % 3 == 0).long()}
    random.seed(seed)
    torch.manual_seed(seed)
    del LOG[:]
    out, tgt = chain(Image.fromarray(img), target)
    nxt = (random.random(), float(torch.rand(1, dtype=torch.float64)))
    log = list(LOG)
    flip = int(log[0][0] == "hflip")
    ops = log[flip:]
    resizes = [o[1:] for o in ops if o[0] == "resize"]
    crops = [o[1:] for o in ops if o[0] == "crop"]
    two = int(len(resizes) == 2)
    params = np.full(9, -1, np.int64)                  # flip, two, size1 h w, crop top left h w (or -1), then size2 below
    params[0], params[1] = flip, two
    if two:
        params[2:4] = resizes[0]
        if crops:
            params[4:8] = crops[0]
    size2 = np.array(resizes[-1], np.int64)
    assert tuple(size2) == out.size[::-1]
    return dict(params=params[:8], size2=size2, out=np.asarray(out), nxt=np.array(nxt, np.float64), n_in=n,
                target={k: np.asarray(v) for k, v in tgt.items()})


def normalize_pad(outs):
    """transformers 4.18 to_numpy_array (rescale by 1/255) + normalize, all float32, then pad_and_create_pixel_mask
    (restated, as in make_golden_preprocess.py)."""
    vs = []
    for o in outs:
        v = o.astype(np.float32) * (1 / 255.0)
        v = v.transpose(2, 0, 1)
        mean, std = np.array(MEAN).astype(v.dtype), np.array(STD).astype(v.dtype)
        vs.append((v - mean[:, None, None]) / std[:, None, None])
    H, W = max(v.shape[1] for v in vs), max(v.shape[2] for v in vs)
    pv = np.zeros((len(vs), 3, H, W), np.float32)
    pm = np.zeros((len(vs), H, W), np.int64)
    for i, v in enumerate(vs):
        pv[i, :, :v.shape[1], :v.shape[2]] = v
        pm[i, :v.shape[1], :v.shape[2]] = 1
    return pv, pm


def pack(cases, prefix):
    """Per-case arrays plus the ragged targets, flattened."""
    out = {prefix + "params": np.stack([c["params"] for c in cases]), prefix + "size2": np.stack([c["size2"] for c in cases]),
           prefix + "next": np.stack([c["nxt"] for c in cases]),
           prefix + "n_out": np.array([len(c["target"]["boxes"]) for c in cases], np.int64),
           prefix + "out_size": np.stack([c["target"]["size"] for c in cases]).astype(np.int64)}
    for f, dt in (("boxes", np.float32), ("area", np.float32), ("class_labels", np.int64), ("iscrowd", np.int64)):
        assert all(c["target"][f].dtype == dt for c in cases), f
        out[prefix + "out_" + f] = np.concatenate([c["target"][f] for c in cases])
    return out


def covered(cases, need_whole=True):
    """Every flip x branch, a crop that drops a box, a crop equal to the whole first resize (small part: with the
    reference's constants it takes two exact draws out of 17 x 17 or more), an identity first resize."""
    combos = {(int(c["params"][0]), int(c["params"][1])) for c in cases}
    drop = any(c["params"][4] >= 0 and len(c["target"]["boxes"]) < c["n_in"] for c in cases)
    whole = any(c["params"][4] >= 0 and tuple(c["params"][6:8]) == tuple(c["params"][2:4]) for c in cases)
    ident = any(c["params"][1] == 1 and tuple(c["params"][2:4]) == tuple(c["shape"]) for c in cases)
    return len(combos) == 4 and drop and (whole or not need_whole) and ident


def small_part(T):
    rng = np.random.default_rng(20261016)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SMALL_SHAPES]
    boxes = [make_boxes(rng, h, w, 6) for h, w in SMALL_SHAPES]
    chains = [build_chain(T, crop, **SMALL) for crop in (False, True)]
    for base in range(0, 100000, 100):          # the first seed base whose cases cover every combination, per variant
        per = []
        for chain in chains:
            cases = [dict(run_case(chain, images[i], boxes[i], base + i), shape=SMALL_SHAPES[i]) for i in range(len(images))]
            per.append(cases)
        if covered(per[1]) and len({(int(c["params"][0]), int(c["params"][1])) for c in per[0]}) == 4 \
                and any(c["params"][1] == 1 and tuple(c["params"][2:4]) == tuple(c["shape"]) for c in per[0]):
            break
    assert covered(per[1]), "no seed base covers the cases"
    out = {"small_pixels": np.concatenate([x.reshape(-1) for x in images]),
           "small_shapes": np.array(SMALL_SHAPES, np.int64), "small_seed_base": base,
           "small_in_boxes": np.stack(boxes)}
    for k, v in SMALL.items():
        out["small_" + k] = np.array(v, np.int64)
    for name, cases in zip(("nocrop_", "crop_"), per):
        out.update(pack(cases, "small_" + name))
        pv, pm = normalize_pad([c["out"] for c in cases])
        out["small_" + name + "pixel_values"], out["small_" + name + "pixel_mask"] = pv, pm.astype(np.uint8)
    return out


def full_part(T):
    rng = np.random.default_rng(7)
    chains = [build_chain(T, crop, **FULL) for crop in (False, True)]
    shapes = [(int(rng.integers(200, 1100)), int(rng.integers(200, 1100))) for _ in range(N_FULL)]
    shapes[1], shapes[3], shapes[5] = (400, 640), (768, 500), (600, 600)          # identity first resizes
    boxes = [make_boxes(rng, h, w, 5) for h, w in shapes]
    for base in range(1000, 100000, 1000):
        cases, shas = [], []
        for i, (h, w) in enumerate(shapes):
            if i < N_SHA:
                img = np.random.default_rng(base + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
            else:
                img = np.zeros((h, w, 3), np.uint8)
            c = dict(run_case(chains[i % 2], img, boxes[i], base + i), shape=(h, w))
            if i < N_SHA:
                shas.append(hashlib.sha256(np.ascontiguousarray(c["out"]).tobytes()).hexdigest())
            cases.append(c)
        sha_cases = cases[:N_SHA]
        if covered(cases[1::2], False) and {(int(c["params"][0]), int(c["params"][1])) for c in sha_cases} >= {(1, 1), (0, 0)} \
                and any(c["params"][4] >= 0 for c in sha_cases):
            break
    assert covered(cases[1::2], False), "no seed base covers the cases"
    out = {"full_shapes": np.array(shapes, np.int64), "full_seed_base": base, "full_in_boxes": np.stack(boxes),
           "full_crop": np.arange(N_FULL) % 2, "full_sha256": np.array(shas)}
    for k, v in FULL.items():
        out["full_" + k] = np.array(v, np.int64)
    out.update(pack(cases, "full_"))
    return out


def main():
    T = load_reference_transform()
    data = small_part(T)
    data.update(full_part(T))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes; seed bases", data["small_seed_base"], data["full_seed_base"])


if __name__ == "__main__":
    main()
