"""RandAugment on the host side (gpu_pipeline.py): config parsing, timm's draw order against the PIL restatement of timm
(tests/_randaug_pil.py), the unchanged draws without --aa, the encoding into icamd_aug_op and the command-line guard."""
import ctypes
import math
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _randaug_pil as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = (0.485, 0.456, 0.406)


def test_parse_rand_augment():
    from imageclassification_amd.gpu_pipeline import RAND_INCREASING_OPS, RAND_OPS, parse_rand_augment
    p = parse_rand_augment("rand-m9-mstd0.5-inc1")
    assert (p.magnitude, p.num_layers, p.magnitude_std, p.magnitude_max, p.prob) == (9, 2, 0.5, None, 0.5)
    assert p.ops == RAND_INCREASING_OPS and len(p.ops) == 15
    p = parse_rand_augment("rand-m7-n3-p0.7")
    assert (p.magnitude, p.num_layers, p.magnitude_std, p.prob) == (7, 3, 0.0, 0.7) and p.ops == RAND_OPS
    assert parse_rand_augment("rand-m9-mstd101").magnitude_std == math.inf
    assert parse_rand_augment("rand-m9-mstd100").magnitude_std == 100.0
    assert parse_rand_augment("rand-m9-inc0").ops == RAND_INCREASING_OPS      # timm tests bool() of the string "0"
    assert parse_rand_augment("rand-mmax20-m15").magnitude_max == 20
    assert parse_rand_augment("rand").magnitude == 10
    assert RAND_OPS == tuple(R.RAND_PLAIN) and RAND_INCREASING_OPS == tuple(R.RAND_INCREASING)
    for bad in ("v0", "original", "augmix-m5", "rand-w0", "rand-m9-tcolor"):
        with pytest.raises(NotImplementedError, match="rand"):
            parse_rand_augment(bad)
    with pytest.raises(ValueError):
        parse_rand_augment("rand-q3")


def _helper_draws(config, n_images, seed):
    """Flips, timm RandAugment's draws (recording what applies; no pixels: the draws never depend on them), then the erase
    draws, per image."""
    random.seed(seed)
    np.random.seed(seed)
    ra = R.rand_augment_transform(config, R.hparams_for(MEAN))
    out = []
    for _ in range(n_images):
        random.random(), random.random()                   # hflip, vflip
        rec = []
        ra(None, rec)
        if random.random() < 0.25:                         # RandomErasing, as draw_train_params draws it
            for _ in range(10):
                target = random.uniform(0.02, 1 / 3) * 64 * 64
                aspect = math.exp(random.uniform(math.log(0.3), math.log(1 / 0.3)))
                h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if 0 < h < 64 and 0 < w < 64:
                    random.randint(0, 64 - h), random.randint(0, 64 - w), random.getrandbits(32)
                    break
        out.append(rec)
    return out, random.getstate(), np.random.get_state()


@pytest.mark.parametrize("config", ["rand-m9-mstd0.5-inc1", "rand-m7-n3-p0.7", "rand-m9-mstd101", "rand-m5-n4-mmax8-p1.0",
                                    "rand-m12-mmax15-mstd1"])
def test_draws_follow_timm(config):
    from imageclassification_amd.gpu_pipeline import draw_train_params, parse_rand_augment
    want, st, npst = _helper_draws(config, 150, 7)
    random.seed(7)
    np.random.seed(7)
    pol = parse_rand_augment(config)
    got = [draw_train_params(64, 0.3, 0.25, aa=pol) for _ in range(150)]
    assert [[(n, tuple(a)) for n, a in g["aug"]] for g in got] == want
    assert all(g["order"] == (-1, -1, -1) for g in got)               # timm drops ColorJitter under auto_augment
    assert random.getstate() == st
    np_now = np.random.get_state()
    assert np.array_equal(np_now[1], npst[1]) and np_now[2:] == npst[2:]
    assert sum(len(g["aug"]) for g in got) > 0
    assert any(g["erase"][2] > 0 for g in got)


def _old_draw_train_params(size, color_jitter=0.3, reprob=0.25, hflip=0.5, vflip=0.5, rng=random):
    """draw_train_params as it was before RandAugment (the yardstick of the aa=None path)."""
    d = {"hflip": int(rng.random() < hflip), "vflip": int(rng.random() < vflip), "order": (-1, -1, -1),
         "factors": (1.0, 1.0, 1.0), "erase": (0, 0, 0, 0), "seed": 0}
    if color_jitter and color_jitter > 0:
        ops = [0, 1, 2]
        rng.shuffle(ops)
        f = [1.0, 1.0, 1.0]
        for op in ops:
            f[op] = rng.uniform(max(0.0, 1 - color_jitter), 1 + color_jitter)
        d["order"], d["factors"] = tuple(ops), tuple(f)
    if reprob > 0 and rng.random() < reprob:
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


def test_draws_without_aa_unchanged():
    from imageclassification_amd.gpu_pipeline import draw_train_params
    for cj, rp in ((0.3, 0.25), (0.0, 0.5), (0.4, 0.0)):
        random.seed(3)
        np.random.seed(3)
        want = [_old_draw_train_params(224, cj, rp) for _ in range(300)]
        st, npst = random.getstate(), np.random.get_state()
        random.seed(3)
        np.random.seed(3)
        got = [draw_train_params(224, cj, rp) for _ in range(300)]
        assert got == want and all("aug" not in g for g in got)
        assert random.getstate() == st and np.array_equal(np.random.get_state()[1], npst[1])


def test_op_frequencies():
    from imageclassification_amd.gpu_pipeline import RAND_INCREASING_OPS, draw_rand_augment, parse_rand_augment
    random.seed(11)
    np.random.seed(11)
    pol = parse_rand_augment("rand-m9-mstd0.5-inc1-n1")
    counts = {n: 0 for n in RAND_INCREASING_OPS}
    applied = 0
    for _ in range(20000):
        d = draw_rand_augment(pol)
        applied += len(d)
        for name, _ in d:
            counts[name] += 1
    assert abs(applied / 20000 - 0.5) < 0.02
    for name, c in counts.items():
        assert abs(c / applied - 1 / 15) < 0.012, (name, c)
    pol = parse_rand_augment("rand-m9-n2-p0.7")
    assert abs(sum(len(draw_rand_augment(pol)) for _ in range(5000)) / 10000 - 0.7) < 0.02


def test_aug_op_struct_matches_header():
    from imageclassification_amd import hip
    header = open(os.path.join(ROOT, "include", "icamd.h")).read()
    documented = int(re.search(r"sizeof\(icamd_aug_op\) == (\d+)", header).group(1))
    assert ctypes.sizeof(hip.AugOp) == documented == hip.AUG_OP_BYTES
    assert hip.AugOp.affine.offset == 16 and hip.AugOp.fill.offset == 12
    for name, kind in hip.AUG_KINDS.items():
        assert re.search(rf"ICAMD_AUG_{name.upper()} = {kind},?\s", header), name
    assert hip.ABI_VERSION == 6


def test_encode_aug_op():
    from imageclassification_amd import hip
    from imageclassification_amd.gpu_pipeline import encode_aug_op, rand_augment_fill
    K = hip.AUG_KINDS
    fill = rand_augment_fill(MEAN)
    assert fill == (124, 116, 104)
    assert rand_augment_fill((0.5, 1.0, 0.0)) == (128, 255, 0)          # round(127.5) -> 128 (half to even), capped at 255
    op = encode_aug_op("Rotate", (0.0,), 37, 37, fill)
    assert op.kind == K["identity"]                                      # Pillow: angle 0 is a copy
    op = encode_aug_op("Rotate", (-0.0,), 37, 37, fill)
    assert op.kind == K["identity"]
    op = encode_aug_op("Rotate", (12.5,), 37, 37, fill)
    a = -math.radians(12.5)
    assert op.kind == K["affine"] and op.affine[0] == round(math.cos(a), 15) and op.affine[1] == round(math.sin(a), 15)
    assert tuple(op.fill) == fill
    c, s_ = round(math.cos(a), 15), round(math.sin(a), 15)
    assert op.affine[2] == c * -18.5 + s_ * -18.5 + 0.0 + 18.5
    op = encode_aug_op("ShearX", (-0.27,), 64, 64, fill)
    assert op.kind == K["affine"] and tuple(op.affine) == (1.0, -0.27, 0.0, 0.0, 1.0, 0.0)
    op = encode_aug_op("TranslateYRel", (0.405,), 64, 37, fill)
    assert tuple(op.affine) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.405 * 37)
    assert encode_aug_op("PosterizeIncreasing", (8,), 8, 8, fill).kind == K["identity"]
    op = encode_aug_op("Posterize", (3,), 8, 8, fill)
    assert (op.kind, op.arg) == (K["posterize"], 3)
    assert (encode_aug_op("SolarizeIncreasing", (26,), 8, 8, fill).kind, encode_aug_op("SolarizeAdd", (99,), 8, 8, fill).arg) == \
        (K["solarize"], 99)
    op = encode_aug_op("SharpnessIncreasing", (1.81,), 8, 8, fill)
    assert op.kind == K["sharpness"] and op.factor == np.float32(1.81)
    for name in ("AutoContrast", "Equalize", "Invert"):
        assert encode_aug_op(name, (), 8, 8, fill).kind == K[name.lower()]
    with pytest.raises(ValueError):
        encode_aug_op("Cutout", (1,), 8, 8, fill)


def test_cli_rejects_unsupported_aa_before_gpu(tmp_path):
    sys.path.insert(0, ROOT)
    import train as T
    for aa, gpu in (("v0", "true"), ("rand-w0", "true"), ("rand-m9-mstd0.5-inc1", "false")):
        args = T.get_args_parser().parse_args(["--model", "resnet18", "--data_path", str(tmp_path / "missing"), "--aa", aa,
                                               "--gpu_aug", gpu])
        with pytest.raises(NotImplementedError):
            T.main(args)
