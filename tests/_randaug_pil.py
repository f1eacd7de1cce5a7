"""timm's RandAugment restated on PIL images (timm auto_augment.py: AugmentOp, RandAugment, rand_augment_transform with the
hparams timm.create_transform passes: img_mean fill, BICUBIC, translate_pct 0.45).  The oracle of tests/test_randaugment_*:
it draws from `random` / numpy's global RNG exactly where timm draws, and every pixel comes from the Pillow call timm makes.
timm is not installed here; this is written from its published source, independently of imageclassification_amd."""
import random
import re

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

_LEVEL_DENOM = 10.0


def _negate(v):
    return -v if random.random() > 0.5 else v


def _rotate_level(level, _h):
    return (_negate(level / _LEVEL_DENOM * 30.0),)


def _enhance_level(level, _h):
    return (level / _LEVEL_DENOM * 1.8 + 0.1,)


def _enhance_increasing_level(level, _h):
    return (max(0.1, 1.0 + _negate(level / _LEVEL_DENOM * 0.9)),)


def _shear_level(level, _h):
    return (_negate(level / _LEVEL_DENOM * 0.3),)


def _translate_rel_level(level, h):
    return (_negate(level / _LEVEL_DENOM * h.get("translate_pct", 0.45)),)


def _posterize_level(level, _h):
    return (int(level / _LEVEL_DENOM * 4),)


def _posterize_increasing_level(level, h):
    return (4 - _posterize_level(level, h)[0],)


def _solarize_level(level, _h):
    return (min(256, int(level / _LEVEL_DENOM * 256)),)


def _solarize_increasing_level(level, h):
    return (256 - _solarize_level(level, h)[0],)


def _solarize_add_level(level, _h):
    return (min(128, int(level / _LEVEL_DENOM * 110)),)


def _affine(img, data, **kw):
    return img.transform(img.size, Image.AFFINE, data, kw["resample"], fillcolor=kw["fillcolor"])


def shear_x(img, f, **kw):
    return _affine(img, (1, f, 0, 0, 1, 0), **kw)


def shear_y(img, f, **kw):
    return _affine(img, (1, 0, 0, f, 1, 0), **kw)


def translate_x_rel(img, pct, **kw):
    return _affine(img, (1, 0, pct * img.size[0], 0, 1, 0), **kw)


def translate_y_rel(img, pct, **kw):
    return _affine(img, (1, 0, 0, 0, 1, pct * img.size[1]), **kw)


def rotate(img, degrees, **kw):
    return img.rotate(degrees, resample=kw["resample"], fillcolor=kw["fillcolor"])


def posterize(img, bits, **_):
    return img if bits >= 8 else ImageOps.posterize(img, bits)


def solarize_add(img, add, thresh=128, **_):
    lut = [min(255, i + add) if i < thresh else i for i in range(256)]
    return img.point(lut * 3)


NAME_TO_OP = {
    "AutoContrast": (lambda img, **_: ImageOps.autocontrast(img), None),
    "Equalize": (lambda img, **_: ImageOps.equalize(img), None),
    "Invert": (lambda img, **_: ImageOps.invert(img), None),
    "Rotate": (rotate, _rotate_level),
    "Posterize": (posterize, _posterize_level),
    "PosterizeIncreasing": (posterize, _posterize_increasing_level),
    "Solarize": (lambda img, t, **_: ImageOps.solarize(img, t), _solarize_level),
    "SolarizeIncreasing": (lambda img, t, **_: ImageOps.solarize(img, t), _solarize_increasing_level),
    "SolarizeAdd": (solarize_add, _solarize_add_level),
    "Color": (lambda img, f, **_: ImageEnhance.Color(img).enhance(f), _enhance_level),
    "ColorIncreasing": (lambda img, f, **_: ImageEnhance.Color(img).enhance(f), _enhance_increasing_level),
    "Contrast": (lambda img, f, **_: ImageEnhance.Contrast(img).enhance(f), _enhance_level),
    "ContrastIncreasing": (lambda img, f, **_: ImageEnhance.Contrast(img).enhance(f), _enhance_increasing_level),
    "Brightness": (lambda img, f, **_: ImageEnhance.Brightness(img).enhance(f), _enhance_level),
    "BrightnessIncreasing": (lambda img, f, **_: ImageEnhance.Brightness(img).enhance(f), _enhance_increasing_level),
    "Sharpness": (lambda img, f, **_: ImageEnhance.Sharpness(img).enhance(f), _enhance_level),
    "SharpnessIncreasing": (lambda img, f, **_: ImageEnhance.Sharpness(img).enhance(f), _enhance_increasing_level),
    "ShearX": (shear_x, _shear_level),
    "ShearY": (shear_y, _shear_level),
    "TranslateXRel": (translate_x_rel, _translate_rel_level),
    "TranslateYRel": (translate_y_rel, _translate_rel_level),
}
RAND_INCREASING = ["AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
                   "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
                   "TranslateXRel", "TranslateYRel"]
RAND_PLAIN = ["AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
              "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"]


def hparams_for(mean):
    return {"img_mean": tuple(min(255, round(255 * m)) for m in mean), "interpolation": Image.BICUBIC}


class AugmentOp:
    def __init__(self, name, prob, magnitude, hparams):
        self.name, self.prob, self.magnitude, self.hparams = name, prob, magnitude, hparams
        self.aug_fn, self.level_fn = NAME_TO_OP[name]
        self.kwargs = {"fillcolor": hparams["img_mean"], "resample": hparams["interpolation"]}
        self.magnitude_std = hparams.get("magnitude_std", 0)
        self.magnitude_max = hparams.get("magnitude_max", None)

    def __call__(self, img, record):
        if self.prob < 1.0 and random.random() > self.prob:
            return img
        magnitude = self.magnitude
        if self.magnitude_std > 0:
            if self.magnitude_std == float("inf"):
                magnitude = random.uniform(0, magnitude)
            elif self.magnitude_std > 0:
                magnitude = random.gauss(magnitude, self.magnitude_std)
        upper_bound = self.magnitude_max or _LEVEL_DENOM
        magnitude = max(0.0, min(magnitude, upper_bound))
        level_args = self.level_fn(magnitude, self.hparams) if self.level_fn is not None else tuple()
        record.append((self.name, tuple(level_args)))
        return None if img is None else self.aug_fn(img, *level_args, **self.kwargs)


class RandAugment:
    def __init__(self, ops, num_layers):
        self.ops, self.num_layers = ops, num_layers

    def __call__(self, img, record=None):
        """img None: draw and record only (timm's draws never depend on the pixels); else the Pillow result."""
        record = [] if record is None else record
        for op in np.random.choice(self.ops, self.num_layers, replace=True):
            img = op(img, record)
        return img


def rand_augment_transform(config_str, hparams):
    magnitude, num_layers, increasing, prob = int(_LEVEL_DENOM), 2, False, 0.5
    hparams = dict(hparams)
    config = config_str.split("-")
    assert config[0] == "rand"
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            mstd = float(val)
            if mstd > 100:
                mstd = float("inf")
            hparams.setdefault("magnitude_std", mstd)
        elif key == "mmax":
            hparams.setdefault("magnitude_max", int(val))
        elif key == "inc":
            if bool(val):
                increasing = True
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "p":
            prob = float(val)
        else:
            raise AssertionError("Unknown RandAugment config section")
    names = RAND_INCREASING if increasing else RAND_PLAIN
    return RandAugment([AugmentOp(n, prob, magnitude, hparams) for n in names], num_layers)


def apply_decisions(img, decisions, mean):
    """The Pillow calls of already-drawn decisions [(name, level args)] on a PIL image (no random draws)."""
    h = hparams_for(mean)
    kw = {"fillcolor": h["img_mean"], "resample": h["interpolation"]}
    for name, args in decisions:
        img = NAME_TO_OP[name][0](img, *args, **kw)
    return img
