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
            from .load_custom import _stream
            dev = pixel_values_list[0].device
            imgs = [x.to(dtype=torch.float32).contiguous() for x in pixel_values_list]
            ptrs = torch.tensor([x.data_ptr() for x in imgs], dtype=torch.int64).to(dev, non_blocking=True)
            hw = torch.tensor([[int(x.shape[-2]), int(x.shape[-1])] for x in imgs], dtype=torch.int32).to(dev, non_blocking=True)
            pv = torch.empty(b, c, mh, mw, dtype=torch.float32, device=dev)
            pm = torch.empty(b, mh, mw, dtype=torch.int64, device=dev)
            _lib.check(_lib.lib().egtr_pad_batch_f32(_stream(), ptrs.data_ptr(), hw.data_ptr(), b, c, mh, mw,
                                                     pv.data_ptr(), pm.data_ptr()), "egtr_pad_batch_f32")
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
    pointer plus offsets).  New tables are appended with one copy; when the buffer is full a larger one replaces it
    (batches already prepared keep the old one alive), so a stream of VG sizes uploads each table once."""
    MAX_INTS = 1 << 26

    def __init__(self, device):
        self.device = device
        self.index = {}
        self.host = np.zeros(0, np.int32)
        self.buf = None

    def lookup(self, pairs):
        new = [p for p in dict.fromkeys(pairs) if p not in self.index]
        if new:
            start = len(self.host)
            if start > self.MAX_INTS:
                self.__init__(self.device)
                return self.lookup(pairs)
            parts = []
            for p in new:
                flat, k, window = _device_table(*p)
                self.index[p] = (start + sum(len(x) for x in parts), k, window)
                parts.append(flat)
            self.host = np.concatenate([self.host] + parts)
            if self.buf is None or self.buf.numel() < len(self.host):
                self.buf = torch.empty(max(2 * len(self.host), 1 << 16), dtype=torch.int32, device=self.device)
                start = 0
            self.buf[start:len(self.host)].copy_(_pinned(self.host[start:]), non_blocking=True)
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
        from .load_custom import _stream
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
        ws = self.workspace.data_ptr() if self.workspace is not None else None
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), entry)(_stream(), self.desc.data_ptr(), B, self.coeffs.data_ptr(),
                                                  self.lut.data_ptr(), H, W, self.prepass_rows, self.prepass_cols, ws,
                                                  pixel_values.data_ptr(), pixel_mask.data_ptr()), entry)
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

    def prepare(self, images, device=None):
        """Upload a batch and everything its launch reads; returns a PreprocessBatch."""
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
        sizes = [self.output_size(h, w) for h, w in orig]

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

        cache = _COEFF_CACHES.setdefault(device, _CoeffCache(device))
        pairs = [p for (h, w), (oh, ow) in zip(orig, sizes) for p in ((w, ow), (h, oh))]
        coeffs, tabs = cache.lookup(pairs)
        desc = np.zeros((len(arrs), _DESC_WORDS), np.int64)
        ws_bytes, prepass_rows, prepass_cols = 0, 0, 0
        for i, (a, (h, w), (oh, ow)) in enumerate(zip(arrs, orig, sizes)):
            if torch.is_tensor(a):
                if a.device != device:
                    raise ValueError(f"image {i} is on {a.device}, the batch runs on {device}")
                if a.stride(2) != 1 or a.stride(1) != 3:
                    a = a.contiguous()
                keep.append(a)
                src, stride = a.data_ptr(), a.stride(0)
            else:
                src, stride = base + offs[i], 3 * w
            (tx, kx, window), (ty, ky, _) = tabs[2 * i], tabs[2 * i + 1]
            route = int(window > PREPROCESS_STAGE_BYTES)
            desc[i] = (src, stride, h, w, oh, ow, tx, kx, ty, ky, route, ws_bytes if route else 0)
            if route:
                ws_bytes += (h * ow * 3 + 15) // 16 * 16
                prepass_rows, prepass_cols = max(prepass_rows, h), max(prepass_cols, ow)
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device) if ws_bytes else None
        key = (device, self.image_mean, self.image_std)
        if key not in _LUTS:
            _LUTS[key] = torch.from_numpy(normalize_lut(self.image_mean, self.image_std)).to(device)
        return PreprocessBatch(device, _pinned(desc).to(device, non_blocking=True), coeffs, _LUTS[key], sizes, orig, workspace,
                               prepass_rows, prepass_cols, keep)
