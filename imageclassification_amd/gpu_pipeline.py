"""Input pipeline on the GPU: the reference's train / eval transforms after JPEG decoding
(/root/reference/datasets.py:121-144; loaders train.py:152-170) as ONE C-ABI call per batch (icamd_image_pipeline).

The host keeps what only it can do -- file I/O and JPEG decoding (PIL) -- and the random DECISIONS (flips, colour-jitter
order and factors, erase box), drawn per image from Python's `random` in the order the host transform of datasets.py
draws them; the pixels never take the per-sample CPU path of the reference (bicubic resize, enhancers, normalisation and
erasing run as HIP kernels with Pillow's exact integer arithmetic).  The result is the fp32 NCHW batch train_one_epoch /
evaluate expect, already on the device.

RandAugment (`--aa rand-...`, timm's rand_augment_transform as timm.create_transform places it: after the flips, before
ToTensor, colour jitter off) follows the same split: `draw_rand_augment` takes timm's decisions on the host from numpy's
global RNG (op choice) and `random` (probability, magnitude noise, sign), `encode_aug_op` turns each applied op into an
icamd_aug_op (affine matrices computed here exactly as Pillow's Python computes them), and icamd_image_pipeline_aug applies
them with Pillow's arithmetic.  timm is not a dependency: its semantics are restated here, unpinned (no timm to test against).
"""
import ctypes
import math
import random
import re

import numpy as np
import torch

from . import hip

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def center_square_box(h, w):
    """timm RandomResizedCrop(scale=(1,1), ratio=(1,1)): whole image if square, else the centred min(W,H) square."""
    side = min(h, w)
    return (h - side) // 2, (w - side) // 2, side, side


# ---- RandAugment (timm auto_augment.py, restated) ----

RAND_INCREASING_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing",
                       "SolarizeAdd", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing",
                       "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RAND_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
            "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
LEVEL_DENOM = 10.0
TRANSLATE_PCT = 0.45          # timm's default hparams['translate_pct']; create_transform does not set it


class RandAugmentPolicy:
    """Parsed `rand-...` config: ops (names, in timm's list order), num_layers, magnitude, magnitude_std (inf = uniform),
    magnitude_max (None = 10), prob."""

    def __init__(self, config, ops, num_layers, magnitude, magnitude_std, magnitude_max, prob):
        self.config, self.ops, self.num_layers = config, ops, num_layers
        self.magnitude, self.magnitude_std, self.magnitude_max, self.prob = magnitude, magnitude_std, magnitude_max, prob

    def __repr__(self):
        return f"RandAugmentPolicy({self.config!r})"


def parse_rand_augment(config):
    """timm rand_augment_transform's config string: `rand` then `-`-separated `<key><value>` sections (m, n, mstd, mmax, inc,
    p).  Only RandAugment is built: other policies and the `w` / `t` keys raise NotImplementedError."""
    if not isinstance(config, str) or not config:
        raise ValueError("empty auto-augment config")
    sections = config.split("-")
    if sections[0] != "rand":
        raise NotImplementedError(f"auto-augment policy '{config}' is not supported: only RandAugment ('rand-...', keys m, n, "
                                  "mstd, mmax, inc, p) runs on the GPU; AutoAugment v0 / original and AugMix are not built")
    magnitude, num_layers, increasing, prob, mstd, mmax = 10, 2, False, 0.5, 0.0, None
    for c in sections[1:]:
        if c.startswith("t") or c.startswith("w"):
            raise NotImplementedError(f"RandAugment key '{c}' of '{config}' is not supported (transform subsets / choice "
                                      "weights); supported keys: m, n, mstd, mmax, inc, p")
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue                                  # timm skips a section without a digit
        key, val = cs[:2]
        if key == "mstd":
            mstd = float(val)
            if mstd > 100:
                mstd = float("inf")                   # uniform magnitude in [0, m]
        elif key == "mmax":
            mmax = int(val)
        elif key == "inc":
            increasing = bool(val) or increasing      # timm tests the STRING: 'inc0' switches it on too
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "p":
            prob = float(val)
        else:
            raise ValueError(f"unknown RandAugment config section '{c}' in '{config}'")
    return RandAugmentPolicy(config, RAND_INCREASING_OPS if increasing else RAND_OPS, num_layers, magnitude, mstd, mmax, prob)


def _negate(v, rng):
    return -v if rng.random() > 0.5 else v


def _level_args(name, level, rng):
    """timm's *_level_to_arg for RandAugment's ops: () for ops without an argument; draws the sign where timm does."""
    if name in ("AutoContrast", "Equalize", "Invert"):
        return ()
    if name == "Rotate":
        return (_negate(level / LEVEL_DENOM * 30.0, rng),)
    if name in ("ShearX", "ShearY"):
        return (_negate(level / LEVEL_DENOM * 0.3, rng),)
    if name in ("TranslateXRel", "TranslateYRel"):
        return (_negate(level / LEVEL_DENOM * TRANSLATE_PCT, rng),)
    if name == "Posterize":
        return (int(level / LEVEL_DENOM * 4),)
    if name == "PosterizeIncreasing":
        return (4 - int(level / LEVEL_DENOM * 4),)
    if name == "Solarize":
        return (min(256, int(level / LEVEL_DENOM * 256)),)
    if name == "SolarizeIncreasing":
        return (256 - min(256, int(level / LEVEL_DENOM * 256)),)
    if name == "SolarizeAdd":
        return (min(128, int(level / LEVEL_DENOM * 110)),)
    if name in ("Color", "Contrast", "Brightness", "Sharpness"):
        return (level / LEVEL_DENOM * 1.8 + 0.1,)
    if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
        return (max(0.1, 1.0 + _negate(level / LEVEL_DENOM * 0.9, rng)),)
    raise ValueError(f"unknown RandAugment op {name}")


def draw_rand_augment(policy, rng=random, np_rng=np.random):
    """One image's RandAugment decisions in timm's draw order: [(op name, level args)] of the ops that apply."""
    out = []
    for k in np_rng.choice(len(policy.ops), policy.num_layers):   # RandAugment.__call__: np.random.choice(ops, n)
        name = policy.ops[int(k)]
        if policy.prob < 1.0 and rng.random() > policy.prob:      # AugmentOp.__call__
            continue
        mag = policy.magnitude
        if policy.magnitude_std > 0:
            if policy.magnitude_std == float("inf"):
                mag = rng.uniform(0, mag)
            else:
                mag = rng.gauss(mag, policy.magnitude_std)
        mag = max(0.0, min(mag, policy.magnitude_max or LEVEL_DENOM))
        out.append((name, _level_args(name, mag, rng)))
    return out


def rand_augment_fill(mean):
    """timm create_transform's hparams['img_mean']: the fill colour of the geometric ops."""
    return tuple(min(255, round(255 * m)) for m in mean)


def _rotate_matrix(degrees, w, h):
    """PIL Image.rotate(degrees, BICUBIC, fillcolor) as (kind, affine data): its fast paths, else its matrix about (w/2, h/2)."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    if angle == 180:                                             # transpose(ROTATE_180): exact pixel centres
        return (-1.0, 0.0, float(w), 0.0, -1.0, float(h))
    if angle in (90, 270) and w == h:                            # transpose(ROTATE_90 / ROTATE_270)
        return (0.0, -1.0, float(w), 1.0, 0.0, 0.0) if angle == 90 else (0.0, 1.0, 0.0, -1.0, 0.0, float(h))
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def encode_aug_op(name, args, w, h, fill, op=None):
    """(op name, level args) -> hip.AugOp for a w x h image (fill: RGB of pixels mapped from outside the image)."""
    op = hip.AugOp() if op is None else op
    op.kind, op.arg, op.factor = hip.AUG_KINDS["identity"], 0, 1.0
    for k in range(3):
        op.fill[k] = int(fill[k])
    affine = None
    if name == "Rotate":
        affine = _rotate_matrix(args[0], w, h)
    elif name == "ShearX":
        affine = (1, args[0], 0, 0, 1, 0)
    elif name == "ShearY":
        affine = (1, 0, 0, args[0], 1, 0)
    elif name == "TranslateXRel":
        affine = (1, 0, args[0] * w, 0, 1, 0)
    elif name == "TranslateYRel":
        affine = (1, 0, 0, 0, 1, args[0] * h)
    elif name in ("AutoContrast", "Equalize", "Invert"):
        op.kind = hip.AUG_KINDS[name.lower()]
    elif name.startswith("Posterize"):
        if args[0] < 8:                                          # timm posterize: bits >= 8 returns the image
            op.kind, op.arg = hip.AUG_KINDS["posterize"], int(args[0])
    elif name.startswith("SolarizeAdd"):
        op.kind, op.arg = hip.AUG_KINDS["solarize_add"], int(args[0])
    elif name.startswith("Solarize"):
        op.kind, op.arg = hip.AUG_KINDS["solarize"], int(args[0])
    else:
        base = name[:-len("Increasing")] if name.endswith("Increasing") else name
        if base not in ("Color", "Contrast", "Brightness", "Sharpness"):
            raise ValueError(f"unknown RandAugment op {name}")
        op.kind, op.factor = hip.AUG_KINDS[base.lower()], float(args[0])
    if affine is not None:
        op.kind = hip.AUG_KINDS["affine"]
        for k in range(6):
            op.affine[k] = float(affine[k])
    return op


def draw_train_params(size, color_jitter=0.3, reprob=0.25, hflip=0.5, vflip=0.5, rng=random, aa=None, np_rng=np.random):
    """One image's random decisions, in the draw order of datasets.TrainTransform (the host path of the same recipe).
    aa (a RandAugmentPolicy or its config string): timm's order -- flips, RandAugment ("aug"), erasing -- with no colour
    jitter, as timm.create_transform builds it when auto_augment is set."""
    d = {"hflip": int(rng.random() < hflip), "vflip": int(rng.random() < vflip), "order": (-1, -1, -1),
         "factors": (1.0, 1.0, 1.0), "erase": (0, 0, 0, 0), "seed": 0}
    if aa:
        policy = parse_rand_augment(aa) if isinstance(aa, str) else aa
        d["aug"] = draw_rand_augment(policy, rng, np_rng)
    elif color_jitter and color_jitter > 0:
        ops = [0, 1, 2]
        rng.shuffle(ops)
        f = [1.0, 1.0, 1.0]
        for op in ops:
            f[op] = rng.uniform(max(0.0, 1 - color_jitter), 1 + color_jitter)
        d["order"], d["factors"] = tuple(ops), tuple(f)
    if reprob > 0 and rng.random() < reprob:      # timm RandomErasing, mode 'pixel', one box, <= 10 attempts
        area = size * size
        for _ in range(10):
            target = rng.uniform(0.02, 1 / 3) * area
            aspect = math.exp(rng.uniform(math.log(0.3), math.log(1 / 0.3)))
            h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < h < size and 0 < w < size:
                d["erase"] = (rng.randint(0, size - h), rng.randint(0, size - w), h, w)
                d["seed"] = rng.getrandbits(32)
                break
    return d


class GpuImagePipeline:
    """uint8 HWC numpy images (any sizes) -> fp32 [B, 3, size, size] on the device."""

    def __init__(self, size, train, color_jitter=0.3, reprob=0.25, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD,
                 device="cuda", auto_augment=""):
        # an unsupported policy fails here, before the GPU is touched
        self.policy = parse_rand_augment(auto_augment) if auto_augment and train else None
        self.fill = rand_augment_fill(mean)
        hip.require_gpu()
        self.lib = hip.load()
        self.size, self.train = int(size), bool(train)
        self.color_jitter, self.reprob = color_jitter, reprob
        self.filter = 1 if train else 0          # bicubic for training (datasets.py:131), torchvision's bilinear for eval
        self.mean = (ctypes.c_float * 3)(*mean)
        self.std = (ctypes.c_float * 3)(*std)
        self.device = torch.device(device)
        self._ws = None
        # two pinned staging buffers (images + descriptor table), alternated per batch; an event recorded behind each
        # upload guards the buffer's reuse, so nothing on the batch path waits for the training kernels queued on the stream
        self._pinned = [None, None]
        self._copied = [None, None]
        self._turn = 0

    def _kmax(self, crop):
        support = 2.0 if self.filter == 1 else 1.0
        return int(math.ceil(support * max(1.0, crop / self.size))) * 2 + 1

    def __call__(self, images, params=None):
        B, S = len(images), self.size
        if params is None:
            params = [draw_train_params(S, self.color_jitter, self.reprob, aa=self.policy) if self.train else None
                      for _ in images]
        descs = (hip.ImageDesc * B)()
        aug = self.policy is not None
        n_ops = max((len(pr.get("aug", ())) for pr in params if pr is not None), default=0) if aug else 0
        ops = (hip.AugOp * max(B * n_ops, 1))()
        total = sum(int(im.shape[0]) * int(im.shape[1]) * 3 for im in images)
        total_al = (total + 255) // 256 * 256
        dsize = ctypes.sizeof(descs) + (ctypes.sizeof(ops) if aug else 0)   # 88 B descriptors, then 8-aligned ops
        slot = self._turn
        self._turn = 1 - slot
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()     # the upload that last read this buffer (two batches ago) has finished
        if self._pinned[slot] is None or self._pinned[slot].numel() < total_al + dsize:
            self._pinned[slot] = torch.empty(max(total_al + dsize, 1 << 20), dtype=torch.uint8).pin_memory()
        host = self._pinned[slot].numpy()
        off, max_crop, kmax = 0, 1, 3
        for i, (im, pr) in enumerate(zip(images, params)):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("images must be uint8 HWC RGB arrays")
            h, w = int(im.shape[0]), int(im.shape[1])
            n = h * w * 3
            host[off:off + n] = im.reshape(-1)
            d = descs[i]
            d.src_offset, d.src_h, d.src_w = off, h, w
            if self.train:
                d.crop_top, d.crop_left, d.crop_h, d.crop_w = center_square_box(h, w)
            else:
                d.crop_top, d.crop_left, d.crop_h, d.crop_w = 0, 0, h, w   # Resize([s, s]): the whole image, squashed
            if pr is not None:
                d.hflip, d.vflip = int(pr["hflip"]), int(pr["vflip"])
                for k in range(3):
                    d.jitter_order[k] = int(pr["order"][k])
                    d.jitter_factor[k] = float(pr["factors"][k])
                d.erase_top, d.erase_left, d.erase_h, d.erase_w = (int(v) for v in pr["erase"])
                d.erase_seed = int(pr["seed"]) & 0xFFFFFFFF
                for k, (name, args) in enumerate(pr.get("aug", ()) if aug else ()):
                    encode_aug_op(name, args, S, S, self.fill, ops[i * n_ops + k])
            else:
                for k in range(3):
                    d.jitter_order[k] = -1
                    d.jitter_factor[k] = 1.0
            max_crop = max(max_crop, d.crop_h)
            kmax = max(kmax, self._kmax(d.crop_h), self._kmax(d.crop_w))
            off += n
        host[total_al:total_al + dsize] = np.frombuffer(bytes(descs) + (bytes(ops) if aug else b""), dtype=np.uint8)
        staged = torch.empty(total_al + dsize, dtype=torch.uint8, device=self.device)
        staged.copy_(self._pinned[slot][:total_al + dsize], non_blocking=True)      # one async upload: images + descriptors
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._copied[slot] = ev
        src, ddev = staged[:total], staged[total_al:]
        if aug:
            need = self.lib.icamd_image_pipeline_aug_workspace_bytes(B, max_crop, S, S, kmax)
        else:
            need = self.lib.icamd_image_pipeline_workspace_bytes(B, max_crop, S, S, kmax)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=self.device)
        if aug:
            hip.check(self.lib.icamd_image_pipeline_aug(src.data_ptr(), ddev.data_ptr(), ddev.data_ptr() + ctypes.sizeof(descs),
                                                        n_ops, B, max_crop, S, S, self.filter, kmax, self.mean, self.std,
                                                        out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                        hip.stream_ptr()), "image_pipeline_aug")
        else:
            hip.check(self.lib.icamd_image_pipeline(src.data_ptr(), ddev.data_ptr(), B, max_crop, S, S, self.filter, kmax,
                                                    self.mean, self.std, out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                    hip.stream_ptr()), "image_pipeline")
        self._last = (B, max_crop, kmax, src, ddev)     # keeps the inputs alive until the stream has consumed them
        return out

    def last_uint8(self):
        """uint8 [B, size, size, 3] image of the last call after resize / flips / jitter / RandAugment (parity tests)."""
        B, max_crop, kmax = self._last[:3]
        p = ctypes.c_void_p()
        hip.check(self.lib.icamd_image_pipeline_u8(self._ws.data_ptr(), B, max_crop, self.size, self.size, kmax, ctypes.byref(p)),
                  "image_pipeline_u8")
        base = self._ws.data_ptr()
        o = p.value - base
        return self._ws[o:o + B * self.size * self.size * 3].view(B, self.size, self.size, 3)


class GpuAugmentLoader:
    """Wraps a loader that yields (list of uint8 HWC arrays, targets) and hands the engine device batches."""

    def __init__(self, loader, pipeline):
        self.loader, self.pipeline = loader, pipeline

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for images, targets in self.loader:
            yield self.pipeline(images), torch.as_tensor(targets, dtype=torch.int64)

    def __getattr__(self, name):
        return getattr(self.__dict__["loader"], name)


def raw_collate(batch):
    """DataLoader collate for RawImageFolder: images stay a list of arrays (sizes differ), targets become a list."""
    return [b[0] for b in batch], [b[1] for b in batch]
