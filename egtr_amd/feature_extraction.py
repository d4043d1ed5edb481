"""Tensor-based counterparts of the reference's feature extractors (model/deformable_detr.py:270-385).

The reference subclasses transformers-4.18 ``DetrFeatureExtractor`` (PIL + torchvision pipeline).  Neither PIL
augmentation nor torchvision is part of the hot path; what the drivers need from these classes is
(1) resize (shorter side ``size``, longer side capped at ``max_size``) + ImageNet normalisation,
(2) ``pad_and_create_pixel_mask`` (collate_fn, train_egtr.py:176-186) and (3) ``post_process`` (dd:273-312).
Those are provided on torch tensors.  The ``WithAugmentor`` variants add the random horizontal flip / random
resize of dd:319-385 in tensor form (crop only for the non-"NoCrop" class).
"""
import math
import random

import numpy as np

import torch
import torch.nn.functional as F

from .util import center_to_corners_format

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _target_size(h, w, size, max_size):
    """DETR resize rule (shorter side -> size, longer side <= max_size)."""
    mn, mx = float(min(h, w)), float(max(h, w))
    if max_size is not None and mx / mn * size > max_size:
        size = int(round(max_size * mn / mx))
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


class DeformableDetrFeatureExtractor:
    model_input_names = ["pixel_values", "pixel_mask"]

    def __init__(self, size=800, max_size=1333, do_resize=True, do_normalize=True, image_mean=IMAGENET_MEAN,
                 image_std=IMAGENET_STD, format="coco_detection", **kwargs):
        self.size, self.max_size = size, max_size
        self.do_resize, self.do_normalize = do_resize, do_normalize
        self.image_mean, self.image_std = tuple(image_mean), tuple(image_std)
        self.format = format

    @classmethod
    def from_pretrained(cls, name_or_path=None, **kwargs):
        return cls(**kwargs)

    # ---- geometry helpers on (C,H,W) float tensors in [0,1]; target boxes are absolute xyxy until normalised
    def _resize(self, image, target, size, max_size=None):
        h, w = image.shape[-2:]
        nh, nw = _target_size(h, w, size, max_size)
        image = F.interpolate(image[None], size=(nh, nw), mode="bilinear", align_corners=False)[0]
        return image, self._resize_target(target, h, w, nh, nw)

    @staticmethod
    def _resize_target(target, h, w, nh, nw):
        if target is not None:
            target = dict(target)
            if "boxes" in target:
                target["boxes"] = target["boxes"] * torch.tensor([nw / w, nh / h, nw / w, nh / h])
            target["size"] = torch.tensor([nh, nw])
        return target

    def _normalize(self, image, target):
        mean = torch.tensor(self.image_mean).view(-1, 1, 1)
        std = torch.tensor(self.image_std).view(-1, 1, 1)
        image = (image - mean) / std
        return image, self._normalize_target(target, *image.shape[-2:])

    @staticmethod
    def _normalize_target(target, h, w):
        if target is not None and "boxes" in target:
            b = target["boxes"]
            cxcywh = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0],
                                  b[:, 3] - b[:, 1]], -1)
            target = dict(target)
            target["boxes"] = cxcywh / torch.tensor([w, h, w, h], dtype=torch.float32)
        return target

    def _augment(self, image, target):
        return image, target

    def __call__(self, images, annotations=None, return_tensors="pt", **kwargs):
        single = torch.is_tensor(images) and images.dim() == 3
        images = [images] if single else list(images)
        annotations = [annotations] if (single and annotations is not None) else annotations
        out_images, out_targets = [], []
        for i, img in enumerate(images):
            img = torch.as_tensor(img, dtype=torch.float32)
            tgt = annotations[i] if annotations is not None else None
            if tgt is not None and "orig_size" not in tgt:
                tgt = dict(tgt, orig_size=torch.tensor(img.shape[-2:]))
            img, tgt = self._augment(img, tgt)
            if self.do_resize:
                img, tgt = self._resize(img, tgt, self.size, self.max_size)
            if self.do_normalize:
                img, tgt = self._normalize(img, tgt)
            out_images.append(img)
            out_targets.append(tgt)
        enc = self.pad_and_create_pixel_mask(out_images)
        if annotations is not None:
            enc["labels"] = out_targets
        return enc

    def pad_and_create_pixel_mask(self, pixel_values_list, return_tensors="pt"):
        """Pad to the largest H, W in the batch (top-left aligned); mask 1 = real pixel, 0 = padding.  Images that already
        live on the GPU (fp32 [C, h, w]) are batched there by one HIP launch (egtr_pad_batch_f32); host images take the
        host loop, like the reference."""
        mh = max(int(x.shape[-2]) for x in pixel_values_list)
        mw = max(int(x.shape[-1]) for x in pixel_values_list)
        b = len(pixel_values_list)
        c = pixel_values_list[0].shape[0]
        if all(torch.is_tensor(x) and x.is_cuda for x in pixel_values_list):
            from . import _lib
            dev = pixel_values_list[0].device
            imgs = [x.to(dtype=torch.float32).contiguous() for x in pixel_values_list]
            ptrs = torch.tensor([x.data_ptr() for x in imgs], dtype=torch.int64).to(dev, non_blocking=True)
            hw = torch.tensor([[int(x.shape[-2]), int(x.shape[-1])] for x in imgs], dtype=torch.int32).to(dev, non_blocking=True)
            pv = torch.empty(b, c, mh, mw, dtype=torch.float32, device=dev)
            pm = torch.empty(b, mh, mw, dtype=torch.int64, device=dev)
            _lib.launch("egtr_pad_batch_f32", ptrs.data_ptr(), hw.data_ptr(), b, c, mh, mw, pv.data_ptr(), pm.data_ptr())
            del imgs   # (alive until the launch was enqueued on the stream that also frees them)
            return {"pixel_values": pv, "pixel_mask": pm}
        pv = torch.zeros(b, c, mh, mw, dtype=torch.float32)
        pm = torch.zeros(b, mh, mw, dtype=torch.int64)
        for i, x in enumerate(pixel_values_list):
            h, w = x.shape[-2:]
            pv[i, :, :h, :w] = torch.as_tensor(x, dtype=torch.float32)
            pm[i, :h, :w] = 1
        return {"pixel_values": pv, "pixel_mask": pm}

    def post_process(self, outputs, target_sizes):
        """dd:273-312: top-100 (query, class) pairs by sigmoid score, boxes to absolute xyxy."""
        out_logits, out_bbox = outputs.logits, outputs.pred_boxes
        if len(out_logits) != len(target_sizes):
            raise ValueError("Make sure that you pass in as many target sizes as the batch dimension of the logits")
        if target_sizes.shape[1] != 2:
            raise ValueError("Each element of target_sizes must contain the size (h, w) of each image of the batch")
        prob = out_logits.sigmoid()
        topk_values, topk_indexes = torch.topk(prob.view(out_logits.shape[0], -1), 100, dim=1)
        scores = topk_values
        topk_boxes = torch.div(topk_indexes, out_logits.shape[2], rounding_mode="floor")
        labels = topk_indexes % out_logits.shape[2]
        boxes = center_to_corners_format(out_bbox)
        boxes = torch.gather(boxes, 1, topk_boxes.unsqueeze(-1).repeat(1, 1, 4))
        img_h, img_w = target_sizes.unbind(1)
        scale_fct = torch.stack([img_w, img_h, img_w, img_h], dim=1).to(boxes.device)
        boxes = boxes * scale_fct[:, None, :]
        return [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(scores, labels, boxes)]


class DeformableDetrFeatureExtractorWithAugmentorNoCrop(DeformableDetrFeatureExtractor):
    """Random horizontal flip + random shorter-side scale (dd:352-385), tensor form."""
    scales = [480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800]
    use_crop = False

    def _hflip(self, image, target):
        image = image.flip(-1)
        if target is not None and "boxes" in target:
            w = image.shape[-1]
            b = target["boxes"]
            target = dict(target, boxes=torch.stack([w - b[:, 2], b[:, 1], w - b[:, 0], b[:, 3]], -1))
        return image, target

    def _augment(self, image, target):
        if random.random() < 0.5:
            image, target = self._hflip(image, target)
        if self.use_crop and random.random() < 0.5:
            image, target = self._resize(image, target, random.choice([400, 500, 600]))
            image, target = self._random_crop(image, target, 384, 600)
        return image, target

    def _resize(self, image, target, size, max_size=None):
        if size == self.size:  # the final resize of the pipeline draws a random scale (dd:340,378)
            size, max_size = random.choice(self.scales), 1333
        return super()._resize(image, target, size, max_size)

    def _random_crop(self, image, target, min_size, max_size):
        h, w = image.shape[-2:]
        cw = random.randint(min_size, min(w, max_size))
        ch = random.randint(min_size, min(h, max_size))
        top, left = random.randint(0, h - ch), random.randint(0, w - cw)
        image = image[:, top:top + ch, left:left + cw]
        if target is not None and "boxes" in target:
            b = target["boxes"] - torch.tensor([left, top, left, top], dtype=torch.float32)
            b = torch.min(b.reshape(-1, 2, 2), torch.tensor([cw, ch], dtype=torch.float32)).clamp(min=0).reshape(-1, 4)
            keep = (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
            target = dict(target, boxes=b[keep], size=torch.tensor([ch, cw]))
            for f in ("class_labels", "area", "iscrowd"):
                if f in target:
                    target[f] = target[f][keep]
        return image, target


class DeformableDetrFeatureExtractorWithAugmentor(DeformableDetrFeatureExtractorWithAugmentorNoCrop):
    use_crop = True


# ---- reference-exact preprocessing on the device (csrc/preprocess.hip, egtr_preprocess_f32 / _bf16) ------------------
# The reference's datasets call transformers-4.18 DetrFeatureExtractor per image: a PIL BILINEAR resize of the uint8 RGB
# image, to_numpy_array's rescale v = f32(u) * f32(1/255), normalize (v - f32(mean)) / f32(std), all float32, then the
# collate's pad_and_create_pixel_mask.  DeformableDetrDeviceFeatureExtractor reproduces those pixel values bit for bit
# from raw uint8 images, in one launch per batch.

PIL_PRECISION_BITS = 22          # Pillow's PRECISION_BITS for 8-bit resampling
PREPROCESS_TILE_W = 128          # include/egtr_hip.h EGTR_PREPROCESS_TILE_W
PREPROCESS_STAGE_BYTES = 16354   # include/egtr_hip.h EGTR_PREPROCESS_STAGE_BYTES
_DESC_WORDS = 12


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (ImagingResample, BILINEAR: support 1) for one axis.

    Returns (bounds int32 [out_size, 2] = (xmin, n), weights int32 [out_size, ksize]): output index xx is
    (2^21 + sum_k weights[xx, k] * in[xmin + k]) >> 22 over k < n, clipped to [0, 255].  The float64 arithmetic follows
    Pillow's C statement by statement (sequential weight sum, round half away from zero to 22 fractional bits)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)       # C's (int) truncates toward zero
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)
    arg = ((x[None, :] + xmin[:, None]) - center[:, None] + 0.5) * ss
    w = np.where(np.abs(arg) < 1.0, 1.0 - np.abs(arg), 0.0)
    w[x[None, :] >= n[:, None]] = 0.0
    ww = np.zeros(out_size, np.float64)
    for k in range(ksize):                  # sequential, like the C loop (np.sum would sum pairwise)
        ww += w[:, k]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(w < 0, -0.5 + w * (1 << PIL_PRECISION_BITS), 0.5 + w * (1 << PIL_PRECISION_BITS))
    return np.stack([xmin, n], 1).astype(np.int32), np.trunc(kk).astype(np.int32)


def normalize_lut(image_mean=IMAGENET_MEAN, image_std=IMAGENET_STD):
    """[3, 256] float32: transformers 4.18 to_numpy_array (rescale by 1/255) + normalize of every uint8 value u."""
    v = np.arange(256, dtype=np.float32) * np.float32(1 / 255.0)
    mean = np.array(image_mean).astype(np.float32)[:, None]
    std = np.array(image_std).astype(np.float32)[:, None]
    return (v[None, :] - mean) / std


def _device_table(in_size, out_size):
    """int32 [out][2] bounds followed by [out][k] weights, k, and the widest input window (bytes of an RGB row) any
    PREPROCESS_TILE_W-column output tile reads.  An axis that keeps its size gets the one-tap identity (Pillow skips
    that pass; 2^21 + 2^22 * u >> 22 == u)."""
    if in_size == out_size:
        bounds = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32)
        weights = np.full((out_size, 1), 1 << PIL_PRECISION_BITS, np.int32)
    else:
        bounds, weights = pil_bilinear_coeffs(in_size, out_size)
    first = bounds[::PREPROCESS_TILE_W, 0].astype(np.int64)
    lastidx = np.minimum(np.arange(len(first)) * PREPROCESS_TILE_W + PREPROCESS_TILE_W - 1, out_size - 1)
    window = int(((bounds[lastidx, 0].astype(np.int64) + bounds[lastidx, 1]) - first).max()) * 3
    return np.concatenate([bounds.ravel(), weights.ravel()]), weights.shape[1], window


def _pinned(array):
    """A host numpy array in pinned memory, for one non-blocking copy to the device."""
    return torch.from_numpy(np.ascontiguousarray(array)).pin_memory()


class _CoeffCache:
    """The coefficient tables of every (in, out) axis seen on one device, in one int32 buffer (the kernel takes one
    pointer plus offsets).  Only the new tables of a batch are built and uploaded, with one copy, so a lookup costs
    O(new tables) however many are cached; no host copy of the buffer is kept.  A full buffer is replaced by one of
    twice the size, filled with a device-to-device copy (batches already prepared keep the old one alive).  At MAX_INTS
    (64 MB) the cache starts afresh instead: random training sizes, crop windows above all, rarely recur, so the memory
    stays bounded and a table that does recur is built again."""
    MAX_INTS = 1 << 24
    MIN_INTS = 1 << 16

    def __init__(self, device):
        self.device = torch.device(device)
        self.index = {}
        self.bounds = {}
        self.used = 0
        self.buf = None

    def lookup(self, pairs):
        new = [p for p in dict.fromkeys(pairs) if p not in self.index]
        if new:
            parts, index, bounds, used = [], {}, {}, self.used
            for p in new:
                flat, k, window = _device_table(*p)
                index[p] = (used, k, window)
                bounds[p] = flat[:2 * p[1]].reshape(-1, 2)
                parts.append(flat)
                used += len(flat)
            if used > self.MAX_INTS and self.used:
                self.__init__(self.device)
                return self.lookup(pairs)
            if self.buf is None or self.buf.numel() < used:
                size = max(min(max(2 * used, self.MIN_INTS), self.MAX_INTS), used)
                grown = torch.empty(size, dtype=torch.int32, device=self.device)
                if self.used:
                    grown[:self.used].copy_(self.buf[:self.used])
                self.buf = grown
            fresh = torch.from_numpy(np.concatenate(parts))
            if self.device.type == "cuda":
                fresh = fresh.pin_memory()
            self.buf[self.used:used].copy_(fresh, non_blocking=True)
            self.index.update(index)
            self.bounds.update(bounds)
            self.used = used
        return self.buf, [self.index[p] for p in pairs]


_COEFF_CACHES = {}
_LUTS = {}


def _as_hwc_uint8(img):
    """An image as (host numpy or device tensor) uint8 [H, W, 3]: PIL images are converted to RGB like the reference's
    loader (Image.open(path).convert("RGB"))."""
    if torch.is_tensor(img):
        arr = img if img.is_cuda else img.numpy()
        ok = img.dtype == torch.uint8
    elif isinstance(img, np.ndarray):
        arr, ok = img, img.dtype == np.uint8
    elif hasattr(img, "convert") and hasattr(img, "size"):
        arr, ok = np.asarray(img.convert("RGB")), True
    else:
        raise TypeError(f"unsupported image type {type(img).__name__}: expected a PIL image or a uint8 HWC array")
    if not ok or arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H, W, 3] image, got {arr.dtype} {tuple(arr.shape)}")
    if arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"empty image {tuple(arr.shape)}")
    return arr


class PreprocessBatch:
    """A prepared batch: images, descriptors, coefficient tables, LUT and workspace resident on the device.  run() is a
    single C call (no allocation when the outputs are given, no synchronisation), so it can be captured into a graph and
    replayed while these tensors live."""

    def __init__(self, device, desc, coeffs, lut, sizes, orig_sizes, workspace, prepass_rows, prepass_cols, keep):
        self.device, self.desc, self.coeffs, self.lut = device, desc, coeffs, lut
        self.sizes, self.orig_sizes = sizes, orig_sizes
        self.workspace, self.prepass_rows, self.prepass_cols = workspace, prepass_rows, prepass_cols
        self._keep = keep
        self.H = max(h for h, _ in sizes)
        self.W = max(w for _, w in sizes)

    def run(self, pixel_values=None, pixel_mask=None, dtype=torch.float32):
        from . import _lib
        B, H, W = len(self.sizes), self.H, self.W
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if pixel_values is None:
            pixel_values = torch.empty(B, 3, H, W, dtype=dtype, device=self.device)
        if pixel_mask is None:
            pixel_mask = torch.empty(B, H, W, dtype=torch.int64, device=self.device)
        if (tuple(pixel_values.shape) != (B, 3, H, W) or pixel_values.dtype != dtype or not pixel_values.is_contiguous()
                or tuple(pixel_mask.shape) != (B, H, W) or pixel_mask.dtype != torch.int64
                or not pixel_mask.is_contiguous()):
            raise ValueError("pixel_values / pixel_mask must be contiguous [B, 3, H, W] / [B, H, W] int64 tensors")
        entry = "egtr_preprocess_f32" if dtype == torch.float32 else "egtr_preprocess_bf16"
        ws = _lib.ptr(self.workspace)
        with torch.cuda.device(self.device):
            _lib.launch(entry, self.desc.data_ptr(), B, self.coeffs.data_ptr(), self.lut.data_ptr(), H, W, self.prepass_rows,
                        self.prepass_cols, ws, pixel_values.data_ptr(), pixel_mask.data_ptr())
        return {"pixel_values": pixel_values, "pixel_mask": pixel_mask}


class DeformableDetrDeviceFeatureExtractor(DeformableDetrFeatureExtractor):
    """The reference's feature extractor + collate pad on the device, bit-identical to transformers 4.18
    DetrFeatureExtractor (do_resize, do_normalize) on PIL images followed by pad_and_create_pixel_mask.

    images: PIL images, uint8 [H, W, 3] numpy arrays or torch tensors (host, or already on the device: read in place).
    Host images are packed into one pinned buffer and uploaded with one copy.  Returns pixel_values [B, 3, H, W]
    (float32, or bfloat16 rounded to nearest even) and pixel_mask [B, H, W] int64 on the device; with annotations also
    "labels", built by the host target code of DeformableDetrFeatureExtractor."""

    def __call__(self, images, annotations=None, return_tensors="pt", device=None, dtype=torch.float32, **kwargs):
        single = not isinstance(images, (list, tuple))
        images = [images] if single else list(images)
        annotations = [annotations] if (single and annotations is not None) else annotations
        batch = self.prepare(images, device)
        enc = batch.run(dtype=dtype)
        if annotations is not None:
            enc["labels"] = self.targets(batch.orig_sizes, annotations)
        return enc

    def output_size(self, h, w):
        return _target_size(h, w, self.size, self.max_size) if self.do_resize else (h, w)

    def targets(self, orig_sizes, annotations):
        """The labels of DeformableDetrFeatureExtractor.__call__ for images of these (h, w): orig_size, box scaling by
        the resized size, cxcywh normalisation."""
        out = []
        for (h, w), tgt in zip(orig_sizes, annotations):
            if tgt is not None and "orig_size" not in tgt:
                tgt = dict(tgt, orig_size=torch.tensor([h, w]))
            nh, nw = self.output_size(h, w)
            if self.do_resize:
                tgt = self._resize_target(tgt, h, w, nh, nw)
            tgt = self._normalize_target(tgt, nh, nw)
            out.append(tgt)
        return out

    def _upload(self, images, device=None):
        """Resolve the device and put the batch's pixels on it.  Returns the device, the (h, w) of every image, its
        (address, row stride in bytes) on the device and the tensors that must outlive the launch."""
        if not self.do_normalize:
            raise NotImplementedError("DeformableDetrDeviceFeatureExtractor always normalises (do_normalize=False)")
        if not images:
            raise ValueError("no images")
        arrs = [_as_hwc_uint8(x) for x in images]
        if device is None:
            on_dev = [a.device for a in arrs if torch.is_tensor(a)]
            device = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"DeformableDetrDeviceFeatureExtractor runs on a GPU, got device {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        orig = [(int(a.shape[0]), int(a.shape[1])) for a in arrs]

        # host images: one pinned buffer, one copy; device images: in place (HWC with packed pixels, any row stride)
        host_idx = [i for i, a in enumerate(arrs) if not torch.is_tensor(a)]
        offs, total = {}, 0
        for i in host_idx:
            offs[i] = total
            total += (arrs[i].size + 15) // 16 * 16
        keep = []
        base = 0
        if host_idx:
            pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            view = pinned.numpy()
            for i in host_idx:
                view[offs[i]:offs[i] + arrs[i].size] = np.ascontiguousarray(arrs[i]).reshape(-1)
            staged = pinned.to(device, non_blocking=True)
            keep.append(staged)
            base = staged.data_ptr()
        srcs = []
        for i, a in enumerate(arrs):
            if torch.is_tensor(a):
                if a.device != device:
                    raise ValueError(f"image {i} is on {a.device}, the batch runs on {device}")
                if a.stride(2) != 1 or a.stride(1) != 3:
                    a = a.contiguous()
                keep.append(a)
                srcs.append((a.data_ptr(), a.stride(0)))
            else:
                srcs.append((base + offs[i], 3 * orig[i][1]))
        return device, orig, srcs, keep

    def _lut(self, device):
        key = (device, self.image_mean, self.image_std)
        if key not in _LUTS:
            _LUTS[key] = torch.from_numpy(normalize_lut(self.image_mean, self.image_std)).to(device)
        return _LUTS[key]

    def prepare(self, images, device=None):
        """Upload a batch and everything its launch reads; returns a PreprocessBatch."""
        device, orig, srcs, keep = self._upload(images, device)
        sizes = [self.output_size(h, w) for h, w in orig]
        cache = _COEFF_CACHES.setdefault(device, _CoeffCache(device))
        pairs = [p for (h, w), (oh, ow) in zip(orig, sizes) for p in ((w, ow), (h, oh))]
        coeffs, tabs = cache.lookup(pairs)
        desc = np.zeros((len(orig), _DESC_WORDS), np.int64)
        ws_bytes, prepass_rows, prepass_cols = 0, 0, 0
        for i, ((src, stride), (h, w), (oh, ow)) in enumerate(zip(srcs, orig, sizes)):
            (tx, kx, window), (ty, ky, _) = tabs[2 * i], tabs[2 * i + 1]
            route = int(window > PREPROCESS_STAGE_BYTES)
            desc[i] = (src, stride, h, w, oh, ow, tx, kx, ty, ky, route, ws_bytes if route else 0)
            if route:
                ws_bytes += (h * ow * 3 + 15) // 16 * 16
                prepass_rows, prepass_cols = max(prepass_rows, h), max(prepass_cols, ow)
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        return PreprocessBatch(device, _pinned(desc).to(device, non_blocking=True), coeffs, self._lut(device), sizes, orig,
                               workspace, prepass_rows, prepass_cols, keep)


# ---- the reference's training augmentation on the device (csrc/augment.hip, egtr_preprocess_augment_f32 / _bf16) -----
# dd:322-385 wrap the PIL chain of model/transform.py around the 4.18 extractor:
#   RandomHorizontalFlip -> RandomSelect(RandomResize(scales, max_size=1333),
#                                        Compose[RandomResize([400, 500, 600]), RandomSizeCrop(384, 600) (not "NoCrop"),
#                                                RandomResize(scales, max_size=1333)])
# Every PIL step is 8-bit.  Here the random draws (sample_augmentation) and the target arithmetic (augment_target) stay
# on the host and are separate from the pixels, which the kernels produce bit-identically from the raw uint8 image.

AUGMENT_SCALES = (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)
AUGMENT_MID_SIZES = (400, 500, 600)
AUGMENT_CROP_RANGE = (384, 600)
_AUG_DESC_WORDS = 17                                  # include/egtr_hip.h EGTR_AUGMENT_DESC_WORDS
_AUG_MIRROR, _AUG_SRC_WS, _AUG_PREPASS = 1, 2, 4      # EGTR_AUGMENT_MIRROR / _SRC_WORKSPACE / _PREPASS


class AugmentParams:
    """What the reference's chain drew for one image: flip (bool), size1 ((h, w) of the first resize, None on the
    one-resize branch), crop ((top, left, h, w) in the first resize's output, or None), size2 ((h, w) of the final
    resize)."""
    __slots__ = ("flip", "size1", "crop", "size2")

    def __init__(self, flip=False, size1=None, crop=None, size2=None):
        self.flip = bool(flip)
        self.size1 = None if size1 is None else (int(size1[0]), int(size1[1]))
        self.crop = None if crop is None else tuple(int(v) for v in crop)
        self.size2 = (int(size2[0]), int(size2[1]))
        if self.size1 is None and self.crop is not None:
            raise ValueError("a crop needs the first resize (size1)")

    def _key(self):
        return self.flip, self.size1, self.crop, self.size2

    def __eq__(self, other):
        return isinstance(other, AugmentParams) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "AugmentParams(flip=%r, size1=%r, crop=%r, size2=%r)" % self._key()

    def window(self):
        """(top, left, h, w): the part of the first resize that the final resize reads."""
        return self.crop if self.crop is not None else (0, 0) + self.size1


def _random_crop_params(h, w, th, tw):
    """torchvision 0.13 transforms.RandomCrop.get_params(img, (th, tw)), restated (torchvision is not a dependency,
    and the restatement is not confirmed against an install): no draw when the crop equals the image, otherwise
    torch.randint for the top and then for the left."""
    if h + 1 < th or w + 1 < tw:
        raise ValueError(f"Required crop size {(th, tw)} is larger then input image size {(h, w)}")
    if w == tw and h == th:
        return 0, 0, h, w
    top = torch.randint(0, h - th + 1, size=(1,)).item()
    left = torch.randint(0, w - tw + 1, size=(1,)).item()
    return top, left, th, tw


def sample_augmentation(h, w, crop, scales=AUGMENT_SCALES, mid_sizes=AUGMENT_MID_SIZES, crop_range=AUGMENT_CROP_RANGE,
                        max_size=1333):
    """Draw one AugmentParams for an h x w image, consuming Python's global `random` and torch's global generator
    exactly as the reference's chain does: random() (flip), random() (branch), then choice(scales), or
    choice(mid_sizes), [randint (crop width), randint (crop height), RandomCrop.get_params], choice(scales)."""
    scales, mid_sizes = list(scales), list(mid_sizes)
    flip = random.random() < 0.5
    if random.random() < 0.5:
        return AugmentParams(flip, None, None, _target_size(h, w, random.choice(scales), max_size))
    size1 = _target_size(h, w, random.choice(mid_sizes), None)
    region = None
    if crop:
        cw = random.randint(crop_range[0], min(size1[1], crop_range[1]))
        ch = random.randint(crop_range[0], min(size1[0], crop_range[1]))
        region = _random_crop_params(size1[0], size1[1], ch, cw)
    wh, ww = region[2:] if region is not None else size1
    return AugmentParams(flip, size1, region, _target_size(wh, ww, random.choice(scales), max_size))


def augment_target(target, h, w, params, normalize=True):
    """The reference's target arithmetic (model/transform.py hflip / resize / crop, float32, step by step) for the h x w
    image `target` belongs to, then the extractor's box normalisation (_normalize_target) unless normalize=False.
    boxes are absolute xyxy float32; `orig_size` is the raw image's."""
    if target is None:
        return None
    target = {k: torch.as_tensor(v) for k, v in target.items()}
    if "orig_size" not in target:
        target["orig_size"] = torch.tensor([h, w])
    ch, cw = h, w                                            # the current image size
    if params.flip and "boxes" in target:
        target["boxes"] = (target["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1])
                           + torch.as_tensor([cw, 0, cw, 0]))

    def resize(nh, nw):
        ratio_width, ratio_height = float(nw) / float(cw), float(nh) / float(ch)
        if "boxes" in target:
            target["boxes"] = target["boxes"] * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
        if "area" in target:
            target["area"] = target["area"] * (ratio_width * ratio_height)
        target["size"] = torch.tensor([nh, nw])
        return nh, nw

    if params.size1 is not None:
        ch, cw = resize(*params.size1)
        if params.crop is not None:
            i, j, rh, rw = params.crop
            target["size"] = torch.tensor([rh, rw])
            if "boxes" in target:
                max_size = torch.as_tensor([rw, rh], dtype=torch.float32)
                cropped = target["boxes"] - torch.as_tensor([j, i, j, i])
                cropped = torch.min(cropped.reshape(-1, 2, 2), max_size).clamp(min=0)
                target["area"] = (cropped[:, 1, :] - cropped[:, 0, :]).prod(dim=1)
                target["boxes"] = cropped.reshape(-1, 4)
                keep = torch.all(cropped[:, 1, :] > cropped[:, 0, :], dim=1)
                for f in ("class_labels", "area", "iscrowd", "boxes"):
                    if f in target:
                        target[f] = target[f][keep]
            ch, cw = rh, rw
    ch, cw = resize(*params.size2)
    if normalize:
        target = DeformableDetrFeatureExtractor._normalize_target(target, ch, cw)
    return target


def _window_bytes(bounds, off, n):
    """The widest input window (bytes of an RGB row) any PREPROCESS_TILE_W-column tile of the output columns
    [off, off + n) reads."""
    first = np.arange(off, off + n, PREPROCESS_TILE_W)
    last = np.minimum(first + PREPROCESS_TILE_W - 1, off + n - 1)
    return int((bounds[last, 0].astype(np.int64) + bounds[last, 1] - bounds[first, 0]).max()) * 3


class AugmentBatch:
    """A prepared augmented batch, like PreprocessBatch: run() is one C call of at most four launches (one when every
    image is on the one-resize branch), with no allocation when the outputs are given and no synchronisation."""

    def __init__(self, device, first, final, coeffs, lut, params, orig_sizes, workspace, extents, keep):
        self.device, self.first, self.final, self.coeffs, self.lut = device, first, final, coeffs, lut
        self.params, self.orig_sizes, self.workspace, self.extents = params, orig_sizes, workspace, extents
        self.sizes = [p.size2 for p in params]
        self._keep = keep
        self.H = max(h for h, _ in self.sizes)
        self.W = max(w for _, w in self.sizes)

    def run(self, pixel_values=None, pixel_mask=None, dtype=torch.float32):
        from . import _lib
        B, H, W = len(self.sizes), self.H, self.W
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if pixel_values is None:
            pixel_values = torch.empty(B, 3, H, W, dtype=dtype, device=self.device)
        if pixel_mask is None:
            pixel_mask = torch.empty(B, H, W, dtype=torch.int64, device=self.device)
        if (tuple(pixel_values.shape) != (B, 3, H, W) or pixel_values.dtype != dtype or not pixel_values.is_contiguous()
                or tuple(pixel_mask.shape) != (B, H, W) or pixel_mask.dtype != torch.int64
                or not pixel_mask.is_contiguous()):
            raise ValueError("pixel_values / pixel_mask must be contiguous [B, 3, H, W] / [B, H, W] int64 tensors")
        entry = "egtr_preprocess_augment_f32" if dtype == torch.float32 else "egtr_preprocess_augment_bf16"
        ws = _lib.ptr(self.workspace)
        first = _lib.ptr(self.first)
        with torch.cuda.device(self.device):
            _lib.launch(entry, first, self.final.data_ptr(), B, self.coeffs.data_ptr(), self.lut.data_ptr(), H, W, *self.extents,
                        ws, pixel_values.data_ptr(), pixel_mask.data_ptr())
        return {"pixel_values": pixel_values, "pixel_mask": pixel_mask}


class DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop(DeformableDetrDeviceFeatureExtractor):
    """The reference's DeformableDetrFeatureExtractorWithAugmentorNoCrop (dd:355-385) + collate pad on the device:
    pixel_values bit-identical to its PIL chain for the same image and the same random draws.

    images as for DeformableDetrDeviceFeatureExtractor (raw uint8; no flip or resize is done by the caller).  `params`
    is one AugmentParams per image; None samples them in batch order with sample_augmentation, from Python's global
    `random` and torch's global generator like the reference.  Sampling happens per batch in the calling process, so a
    seeded run is comparable with the reference per draw sequence, not per epoch of a multi-worker loader (whose
    workers each hold their own generator state).  `size` is ignored, as in the reference's override; `max_size` caps
    the random-scale resizes."""
    use_crop = False

    def __init__(self, size=800, max_size=1333, scales=AUGMENT_SCALES, mid_sizes=AUGMENT_MID_SIZES,
                 crop_range=AUGMENT_CROP_RANGE, **kwargs):
        super().__init__(size=size, max_size=max_size, **kwargs)
        self.scales, self.mid_sizes, self.crop_range = tuple(scales), tuple(mid_sizes), tuple(crop_range)

    def sample(self, h, w):
        return sample_augmentation(h, w, self.use_crop, self.scales, self.mid_sizes, self.crop_range, self.max_size)

    def __call__(self, images, annotations=None, params=None, return_tensors="pt", device=None, dtype=torch.float32,
                 **kwargs):
        single = not isinstance(images, (list, tuple))
        images = [images] if single else list(images)
        annotations = [annotations] if (single and annotations is not None) else annotations
        if single and isinstance(params, AugmentParams):
            params = [params]
        batch = self.prepare(images, device, params)
        enc = batch.run(dtype=dtype)
        if annotations is not None:
            enc["labels"] = [augment_target(t, h, w, p)
                             for t, (h, w), p in zip(annotations, batch.orig_sizes, batch.params)]
        return enc

    @staticmethod
    def _check(p):
        for name, s in (("size1", p.size1), ("size2", p.size2)):
            if s is not None and (s[0] < 1 or s[1] < 1):
                raise ValueError(f"{name} {s} must be positive")
        if p.crop is not None:
            top, left, ch, cw = p.crop
            if top < 0 or left < 0 or ch < 1 or cw < 1 or top + ch > p.size1[0] or left + cw > p.size1[1]:
                raise ValueError(f"crop {p.crop} leaves the first resize {p.size1}")

    def prepare(self, images, device=None, params=None):
        """Upload a batch and everything its launches read; returns an AugmentBatch."""
        device, orig, srcs, keep = self._upload(images, device)
        if params is None:
            params = [self.sample(h, w) for h, w in orig]
        params = list(params)
        if len(params) != len(orig):
            raise ValueError(f"{len(params)} AugmentParams for {len(orig)} images")
        pairs = []
        for (h, w), p in zip(orig, params):
            self._check(p)
            if p.size1 is None:
                pairs += [(w, p.size2[1]), (h, p.size2[0])] * 2
            else:
                _, _, wh, ww = p.window()
                pairs += [(w, p.size1[1]), (h, p.size1[0]), (ww, p.size2[1]), (wh, p.size2[0])]
        cache = _COEFF_CACHES.setdefault(device, _CoeffCache(device))
        coeffs, tabs = cache.lookup(pairs)
        first = np.zeros((len(orig), _AUG_DESC_WORDS), np.int64)
        final = np.zeros((len(orig), _AUG_DESC_WORDS), np.int64)
        ws = [0]
        ext = [0] * 6      # first rows / cols, prepass rows / cols of the first pass, of the final pass

        def region(nbytes):
            off = ws[0]
            ws[0] += (nbytes + 15) // 16 * 16
            return off

        def one_pass(src, stride, in_h, in_w, full, window, flags, tab_x, tab_y, pair_x, pair_y, e):
            """The descriptor of one resize pass; routes it through the horizontal prepass (of the input rows the window
            reads) when a tile's input window does not fit the LDS stage."""
            top, left, oh, ow = window
            pre = 0
            if _window_bytes(cache.bounds[pair_x], left, ow) > PREPROCESS_STAGE_BYTES:
                flags |= _AUG_PREPASS
                by = cache.bounds[pair_y]
                rows = int(by[top + oh - 1, 0]) + int(by[top + oh - 1, 1]) - int(by[top, 0])
                pre = region(rows * ow * 3)
                ext[e], ext[e + 1] = max(ext[e], rows), max(ext[e + 1], ow)
            return (src, stride, in_h, in_w, oh, ow, tab_x[0], tab_x[1], tab_y[0], tab_y[1], left, top, full[1], full[0],
                    flags, pre, 0)

        for i, ((src, stride), (h, w), p) in enumerate(zip(srcs, orig, params)):
            t = tabs[4 * i:4 * i + 4]
            pp = pairs[4 * i:4 * i + 4]
            mirror = _AUG_MIRROR if p.flip else 0
            if p.size1 is None:
                final[i] = one_pass(src, stride, h, w, p.size2, (0, 0) + p.size2, mirror, t[0], t[1], pp[0], pp[1], 4)
                continue
            window = p.window()
            d = list(one_pass(src, stride, h, w, p.size1, window, mirror, t[0], t[1], pp[0], pp[1], 2))
            d[16] = region(window[2] * window[3] * 3)
            first[i] = d
            ext[0], ext[1] = max(ext[0], window[2]), max(ext[1], window[3])
            final[i] = one_pass(d[16], 3 * window[3], window[2], window[3], p.size2, (0, 0) + p.size2, _AUG_SRC_WS,
                                t[2], t[3], pp[2], pp[3], 4)
        workspace = torch.empty(ws[0], dtype=torch.uint8, device=device) if ws[0] else None
        descs = _pinned(np.stack([first, final])).to(device, non_blocking=True)
        return AugmentBatch(device, descs[0] if ext[0] else None, descs[1], coeffs, self._lut(device), params, orig,
                            workspace, tuple(ext), keep + [descs])


class DeformableDetrDeviceFeatureExtractorWithAugmentor(DeformableDetrDeviceFeatureExtractorWithAugmentorNoCrop):
    """The reference's DeformableDetrFeatureExtractorWithAugmentor (dd:322-352): the chain above with
    RandomSizeCrop(384, 600) between the two resizes of the second branch."""
    use_crop = True
