"""RandAugment on the GPU (icamd_image_pipeline_aug) against Pillow itself, through the PIL restatement of timm in
tests/_randaug_pil.py: every op of both lists at several magnitudes, signs, sizes and image kinds, chains, a full drawn batch,
the unchanged plain pipeline, and the command line.  uint8 images are compared EXACTLY, the normalised tensor to 1e-6."""
import json
import math
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _randaug_pil as R  # noqa: E402
from oracle import image_ref as I  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ALL_OPS = sorted(set(R.RAND_INCREASING) | set(R.RAND_PLAIN))
SIGNED = {"Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "ColorIncreasing", "ContrastIncreasing",
          "BrightnessIncreasing", "SharpnessIncreasing"}


class _Sign:
    """rng stand-in for the level functions: random() > 0.5 negates."""

    def __init__(self, neg):
        self.v = 0.9 if neg else 0.1

    def random(self):
        return self.v


def _kinds(size, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    noise = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
    grad = np.stack([yy * 255 // (size - 1), xx * 255 // (size - 1), (yy * 3 + xx * 5) % 256], -1).astype(np.uint8)
    two = np.where(((yy // 5 + xx // 7) % 2)[..., None] == 1, np.array([200, 30, 90]), np.array([20, 180, 60])).astype(np.uint8)
    const = np.full((size, size, 3), (77, 140, 201), np.uint8)
    return [noise, grad, two, const]


def _params(decisions):
    return {"hflip": 0, "vflip": 0, "order": (-1, -1, -1), "factors": (1.0, 1.0, 1.0), "erase": (0, 0, 0, 0), "seed": 0,
            "aug": decisions}


def _run(pipe, imgs, params):
    out = pipe(imgs, params)
    torch.cuda.synchronize()
    return out, pipe.last_uint8().cpu().numpy()


def _pil(a, decisions):
    return np.asarray(R.apply_decisions(Image.fromarray(a), decisions, MEAN))


@pytest.mark.parametrize("size", [224, 64, 37])
def test_every_op_exact(size):
    from imageclassification_amd.gpu_pipeline import GpuImagePipeline, _level_args
    cases = []
    for name in ALL_OPS:
        for mag in (0, 1, 5, 9, 10):
            for neg in ((False, True) if name in SIGNED else (False,)):
                cases.append([(name, _level_args(name, mag, _Sign(neg)))])
    cases.append([("Rotate", (0.0,))])
    cases.append([("Rotate", (-0.0,))])
    kinds = _kinds(size, size)
    imgs, params = [], []
    for c in cases:
        for a in kinds:
            imgs.append(a)
            params.append(_params(c))
    pipe = GpuImagePipeline(size, True, reprob=0, auto_augment="rand-m9-mstd0.5-inc1")
    _, u8 = _run(pipe, imgs, params)
    bad = []
    for k, (a, p) in enumerate(zip(imgs, params)):
        ref = _pil(a, p["aug"])
        if not np.array_equal(u8[k], ref):
            bad.append((p["aug"], k % 4, int((u8[k] != ref).sum()), int(np.abs(u8[k].astype(int) - ref).max())))
    assert not bad, (len(bad), bad[:8])


def test_chains_and_resize_path():
    """Ops in sequence where order matters, behind the resize / flips of the pipeline; chains of different lengths in one
    batch (identity slots), odd and even slot counts (the resize then writes the other ping-pong buffer)."""
    from imageclassification_amd.gpu_pipeline import GpuImagePipeline, center_square_box
    chains = [
        [("Rotate", (21.0,)), ("Equalize", ())],
        [("ShearX", (0.27,)), ("SharpnessIncreasing", (1.72,))],
        [("TranslateXRel", (-0.3,)), ("AutoContrast", ()), ("ContrastIncreasing", (0.37,))],
        [("Solarize", (100,)), ("ShearY", (-0.24,)), ("Color", (1.9,))],
        [("Sharpness", (0.3,)), ("Rotate", (-13.0,)), ("Sharpness", (1.9,))],
        [("ShearY", (0.3,)), ("Equalize", ()), ("Invert", ())],
        [("PosterizeIncreasing", (2,)), ("Brightness", (1.63,))],
        [],
        [("SolarizeAdd", (110,))],
        [("Contrast", (0.1,)), ("AutoContrast", ())],
    ]
    rng = np.random.RandomState(5)
    sizes = [(int(rng.randint(60, 300)), int(rng.randint(60, 300))) for _ in chains]
    imgs = []
    for k, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([yy * 255 // (h - 1), xx * 255 // (w - 1), (yy + 2 * xx) % 256], -1) + rng.randint(0, 30, (h, w, 3))
        imgs.append(np.clip(a, 0, 255).astype(np.uint8))
    pipe = GpuImagePipeline(96, True, auto_augment="rand-m9-mstd0.5-inc1")
    for sel in (list(range(len(chains))), [0, 1, 6, 8], [8, 9]):
        params = []
        for k in sel:
            p = _params(chains[k])
            p["hflip"], p["vflip"] = k & 1, (k >> 1) & 1
            params.append(p)
        out, u8 = _run(pipe, [imgs[k] for k in sel], params)
        for j, k in enumerate(sel):
            t, l, ch, cw = center_square_box(*imgs[k].shape[:2])
            x = I.resize_u8(imgs[k][t:t + ch, l:l + cw], 96, 96, "bicubic")
            x = x[:, ::-1] if params[j]["hflip"] else x
            x = np.ascontiguousarray(x[::-1] if params[j]["vflip"] else x)
            ref = _pil(x, chains[k])
            assert np.array_equal(u8[j], ref), (k, chains[k], int((u8[j] != ref).sum()))
            assert np.allclose(out[j].cpu().numpy(), I.to_tensor_normalize(ref, MEAN, STD), atol=1e-6, rtol=0)


def test_full_batch_drawn_policy():
    from imageclassification_amd.gpu_pipeline import GpuImagePipeline, center_square_box, draw_train_params
    rng = np.random.RandomState(21)
    imgs = []
    for _ in range(256):
        h, w = int(rng.randint(300, 520)), int(rng.randint(300, 520))
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([yy * 255 // h, xx * 255 // w, (yy + xx) % 256], -1) + rng.randint(0, 40, (h, w, 3))
        imgs.append(np.clip(a, 0, 255).astype(np.uint8))
    pipe = GpuImagePipeline(224, True, 0.3, 0.25, auto_augment="rand-m9-mstd0.5-inc1")
    random.seed(4)
    np.random.seed(4)
    params = [draw_train_params(224, 0.3, 0.25, aa=pipe.policy) for _ in imgs]
    assert sum(len(p["aug"]) for p in params) > 200 and any(p["erase"][2] for p in params)
    out, u8 = _run(pipe, imgs, params)
    assert tuple(out.shape) == (256, 3, 224, 224) and torch.isfinite(out).all()
    ranked = sorted(range(256), key=lambda k: -len(params[k]["aug"]))
    check = ranked[:4] + [k for k in range(256) if params[k]["erase"][2]][:2]
    for k in check:
        t, l, ch, cw = center_square_box(*imgs[k].shape[:2])
        x = I.resize_u8(imgs[k][t:t + ch, l:l + cw], 224, 224, "bicubic")
        x = x[:, ::-1] if params[k]["hflip"] else x
        x = np.ascontiguousarray(x[::-1] if params[k]["vflip"] else x)
        ref = _pil(x, params[k]["aug"])
        assert np.array_equal(u8[k], ref), (k, params[k]["aug"])
        want = I.to_tensor_normalize(ref, MEAN, STD)
        got = out[k].cpu().numpy().copy()
        top, left, eh, ew = params[k]["erase"]
        if eh:
            got[:, top:top + eh, left:left + ew] = want[:, top:top + eh, left:left + ew]
        assert np.allclose(got, want, atol=1e-6, rtol=0), k
    out2 = pipe(imgs, params)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


def test_plain_pipeline_unchanged_and_identity_slots():
    """Without --aa the pipeline calls icamd_image_pipeline as before; the aug entry with identity slots gives the same bits."""
    from imageclassification_amd.gpu_pipeline import GpuImagePipeline, draw_train_params
    rng = np.random.RandomState(8)
    imgs = [rng.randint(0, 256, (int(rng.randint(40, 200)), int(rng.randint(40, 200)), 3)).astype(np.uint8) for _ in range(12)]
    random.seed(2)
    params = [draw_train_params(72, 0.3, 0.5) for _ in imgs]
    plain = GpuImagePipeline(72, True)
    assert plain.policy is None
    out0, u0 = _run(plain, imgs, params)
    aug = GpuImagePipeline(72, True, auto_augment="rand-m9-mstd0.5-inc1")
    for slots in (0, 1, 2, 3):
        ps = [dict(p, aug=[("Rotate", (0.0,))] * slots) for p in params]
        out1, u1 = _run(aug, imgs, ps)
        assert torch.equal(out0, out1) and np.array_equal(u0, u1), slots


def _make_folder(root, n_per_class=48, hw=48):
    rng = np.random.RandomState(1)
    for ci, cls in enumerate(("cat", "dog")):
        os.makedirs(os.path.join(root, cls))
        for i in range(n_per_class):
            a = rng.randint(0, 90, (hw, hw, 3)).astype(np.uint8)
            a[..., ci] += 150
            Image.fromarray(a).save(os.path.join(root, cls, f"{i:03d}.png"))


def test_train_cli_rand_augment(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import train as T
    data = tmp_path / "data"
    os.makedirs(data)
    _make_folder(str(data))
    work = tmp_path / "work"
    os.makedirs(work / "train_cls" / "output")
    monkeypatch.chdir(work)
    argv = ["--model", "resnet18", "--data_path", str(data), "--batch_size", "16", "--epochs", "2", "--input_size", "48",
            "--num_workers", "0", "--mixup", "0", "--warmup_epochs", "1", "--lr", "2e-3", "--model_ema", "false",
            "--reprob", "0.25", "--gpu_aug", "true", "--auto_resume", "false"]
    stats = T.main(T.get_args_parser().parse_args(argv + ["--aa", "rand-m9-mstd0.5-inc1"]))
    lines = [json.loads(l) for l in open(work / "train_cls" / "log.txt")]
    assert [l["epoch"] for l in lines] == [0, 1]
    assert all(math.isfinite(l["train_loss"]) for l in lines) and math.isfinite(stats["test_loss"])
    with pytest.raises(NotImplementedError):
        T.main(T.get_args_parser().parse_args(argv + ["--aa", "v0"]))
