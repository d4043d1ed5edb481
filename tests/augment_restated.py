"""A numpy restatement of the augmented pixel path, written the way csrc/augment.hip computes it.

A resize pass is pil_resample_restated.resample_axis's arithmetic (Pillow's 8-bit pass over pil_bilinear_coeffs) with the
two things the kernels add: only the table rows of a window [off, off + n) are produced, and a mirrored pass reads input
pixel in_size - 1 - (xmin + k) through the table of the unflipped size, so the flipped image is never built.  An axis
that keeps its size uses the one-tap identity, like the kernels' table.  resample_axis itself has neither a window nor a
mirror; tests/test_augment_cpu.py pins pass_axis to it on whole unmirrored axes."""
import numpy as np

import pil_resample_restated as R
from egtr_amd.feature_extraction import AugmentParams, pil_bilinear_coeffs

PRECISION_BITS = R.PRECISION_BITS


def pass_axis(a, out_size, axis, off=0, n=None, mirror=False):
    """Outputs [off, off + n) of the Pillow pass in_size -> out_size along `axis` of a uint8 array, the input read
    mirrored along that axis when `mirror`."""
    in_size = a.shape[axis]
    n = out_size - off if n is None else n
    assert 0 <= off and n >= 1 and off + n <= out_size
    a = np.moveaxis(a, axis, 0)
    if in_size == out_size:                                   # the one-tap identity table
        idx = np.arange(off, off + n)
        out = a[in_size - 1 - idx if mirror else idx]
        return np.moveaxis(out, 0, axis)
    bounds, weights = pil_bilinear_coeffs(in_size, out_size)
    bounds, weights = bounds[off:off + n].astype(np.int64), weights[off:off + n].astype(np.int64)
    a = a.astype(np.int64)
    acc = np.full((n,) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for k in range(weights.shape[1]):
        live = k < bounds[:, 1]
        src = np.where(live, bounds[:, 0] + k, 0)
        if mirror:
            src = in_size - 1 - src
        w = np.where(live, weights[:, k], 0)
        acc += w.reshape((-1,) + (1,) * (a.ndim - 1)) * a[src]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_window(img, full, window, mirror):
    """Rows [top, top + h) x columns [left, left + w) of PIL's resize of the (mirrored) uint8 [H, W, 3] image to
    full = (h, w): the horizontal pass over the window's columns, then the vertical pass over its rows."""
    top, left, h, w = window
    x = pass_axis(img, full[1], 1, left, w, mirror)
    return pass_axis(x, full[0], 0, top, h, False)


def augment_image(img, p):
    """The final uint8 [h2, w2, 3] image of the chain for one AugmentParams."""
    if p.size1 is None:
        return resize_window(img, p.size2, (0, 0) + p.size2, p.flip)
    first = resize_window(img, p.size1, p.window(), p.flip)       # the workspace bytes: the crop window only
    return resize_window(first, p.size2, (0, 0) + p.size2, False)


def augment_batch(images, params):
    """pixel_values [B, 3, H, W] float32 and pixel_mask [B, H, W] int64 of a batch."""
    outs = [R.normalize(augment_image(img, p)) for img, p in zip(images, params)]
    H = max(o.shape[1] for o in outs)
    W = max(o.shape[2] for o in outs)
    pv = np.zeros((len(outs), 3, H, W), np.float32)
    pm = np.zeros((len(outs), H, W), np.int64)
    for i, o in enumerate(outs):
        pv[i, :, :o.shape[1], :o.shape[2]] = o
        pm[i, :o.shape[1], :o.shape[2]] = 1
    return pv, pm


def pillow_chain(img, p):
    """The same parameters through Pillow itself: transpose / resize / crop / resize."""
    from PIL import Image
    im = Image.fromarray(img)
    if p.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if p.size1 is not None:
        im = im.resize(p.size1[::-1], Image.BILINEAR)
        if p.crop is not None:
            top, left, h, w = p.crop
            im = im.crop((left, top, left + w, top + h))
    return np.asarray(im.resize(p.size2[::-1], Image.BILINEAR))


def seeded_images(shapes, seed):
    """uint8 [h, w, 3] test images: smooth gradients plus noise, so realistic neighbourhoods, every byte value and
    clipping on both ends."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in shapes:
        yy, xx = np.meshgrid(np.linspace(-40, 300, h), np.linspace(-40, 300, w), indexing="ij")
        base = np.stack([yy, xx, (yy + xx) / 2], -1) + rng.normal(0, 30, (h, w, 3))
        out.append(np.clip(base, 0, 255).astype(np.uint8))
    return out


# ---- the committed fixture (tests/golden/augment.npz, written by tests/golden/make_golden_augment.py) ----------------

def fixture_params(row, size2):
    """AugmentParams from a fixture row (flip, two, size1 h w, crop top left h w or -1) and its final size."""
    flip, two = bool(row[0]), bool(row[1])
    size1 = (int(row[2]), int(row[3])) if two else None
    crop = tuple(int(v) for v in row[4:8]) if two and row[4] >= 0 else None
    return AugmentParams(flip, size1, crop, (int(size2[0]), int(size2[1])))


def fixture_constants(g, part):
    return dict(scales=[int(v) for v in g[part + "_scales"]], mid_sizes=[int(v) for v in g[part + "_mid_sizes"]],
                crop_range=tuple(int(v) for v in g[part + "_crop_range"]), max_size=int(g[part + "_max_size"]))


def small_images(g):
    images, o = [], 0
    for h, w in g["small_shapes"]:
        images.append(g["small_pixels"][o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    assert o == g["small_pixels"].size
    return images


def input_target(boxes):
    """The annotation the generator fed to the chain for these boxes."""
    import torch
    n = len(boxes)
    return {"boxes": torch.from_numpy(np.array(boxes, np.float32)), "class_labels": torch.arange(n) % 7,
            "area": torch.from_numpy((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])),
            "iscrowd": (torch.arange(n) % 3 == 0).long()}


def output_targets(g, prefix):
    """The chain's output targets of every case under `prefix` (before the extractor's box normalisation)."""
    import torch
    outs, o = [], 0
    for i, n in enumerate(g[prefix + "n_out"]):
        n = int(n)
        t = {f: torch.from_numpy(g[prefix + "out_" + f][o:o + n]) for f in ("boxes", "area", "class_labels", "iscrowd")}
        t["size"] = torch.from_numpy(g[prefix + "out_size"][i])
        outs.append(t)
        o += n
    return outs
