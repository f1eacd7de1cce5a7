"""Generates tests/golden/arena_layouts.json: one SHA-256 per model over everything the flat-arena protocol fixes.

Run at the commit whose layout is to be pinned (no GPU needed):
    python tests/golden/make_arena_layouts.py

The models construct on the CPU once hip.require_gpu / hip.load / hip.stream_ptr are replaced (`install_stubs`): the constructor
only lays out the arenas, plans the filter transposes and loads the initial weights, and every library call it makes returns 0
from the stand-in.  What is hashed (`layout_record`): the ordered state_dict() keys (buffers included), every parameter's
(name, offset, numel, torch shape, padded shape) -- the torch shape as state_dict() returns it --, n_params, the sizes of shadow_t
and buffer_arena, and the transpose tables _tr_descs / _tr_tjobs / _tr_jobs with their counts.  The optimizer's buckets, the EMA,
DDP's ranges and checkpoints all address parameters by these offsets, so a model whose hash moves does not interchange with the
ones before it.  tests/test_arena_cpu.py rebuilds every model and compares.
"""
import hashlib
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NUM_CLASSES = 10      # the head is padded to 64 rows
# id -> (module, class, constructor arguments)
MODELS = {
    "resnet18": ("nets", "ResNet", {"arch": "resnet18"}),
    "resnet50": ("nets", "ResNet", {"arch": "resnet50"}),
    "resnext50_32x4d": ("nets", "ResNet", {"arch": "resnext50_32x4d"}),
    "seresnet50": ("nets", "ResNet", {"arch": "seresnet50"}),
    "resnet50d": ("nets", "ResNet", {"arch": "resnet50d"}),
    "seresnext26d_32x4d": ("nets", "ResNet", {"arch": "seresnext26d_32x4d"}),
    "convnext_test": ("convnext", "ConvNeXt", {"arch": "convnext_test"}),
    "convnext_tiny": ("convnext", "ConvNeXt", {"arch": "convnext_tiny"}),
    "vit_tiny_test": ("vit", "VisionTransformer", {"arch": "vit_tiny_test"}),
    "vit_base_patch16_224": ("vit", "VisionTransformer", {"arch": "vit_base_patch16_224"}),
    "vit_small_patch16_384": ("vit", "VisionTransformer", {"arch": "vit_small_patch16_384"}),
    "swin_test": ("swin", "SwinTransformer", {"arch": "swin_test", "img_size": 56}),
    "swin_tiny_patch4_window7_224": ("swin", "SwinTransformer", {"arch": "swin_tiny_patch4_window7_224"}),
}


class NullLib:
    """Stands in for libicamd.so: every entry returns 0 (success, or a workspace of no bytes)."""

    def __getattr__(self, name):
        return lambda *args: 0


def install_stubs(setattr_fn=setattr):
    """The three replacements under which the models build without a GPU; a test passes monkeypatch.setattr."""
    from imageclassification_amd import hip
    setattr_fn(hip, "require_gpu", lambda: None)
    setattr_fn(hip, "load", lambda: NullLib())
    setattr_fn(hip, "stream_ptr", lambda: 0)


def build_model(model_id):
    module, cls, kwargs = MODELS[model_id]
    mod = importlib.import_module("imageclassification_amd." + module)
    return getattr(mod, cls)(num_classes=NUM_CLASSES, device="cpu", seed=0, **kwargs)


def layout_record(model):
    sd = model.state_dict()
    ntjobs, njobs = model._tr_ntjobs, getattr(model, "_tr_njobs", 0)
    return {
        "state_dict_keys": list(sd.keys()),
        "params": [[p.name, p.offset, p.numel, list(sd[p.name].shape), list(p.padded_shape)] for p in model.params.values()],
        "n_params": model.n_params,
        "shadow_t": model.shadow_t.numel(),
        "buffer_arena": model.buffer_arena.numel(),
        "tr_descs": model._tr_descs.tolist(),
        "tr_ntjobs": ntjobs,
        "tr_tjobs": model._tr_tjobs.tolist()[:ntjobs],
        "tr_njobs": njobs,
        "tr_jobs": model._tr_jobs.tolist()[:njobs] if njobs else [],
    }


def layout_hash(model):
    blob = json.dumps(layout_record(model), sort_keys=True, separators=(",", ":"))
    return hashlib.sha256(blob.encode()).hexdigest()


def main():
    install_stubs()
    out = {"generator": "tests/golden/make_arena_layouts.py", "num_classes": NUM_CLASSES, "models": {}}
    for model_id in MODELS:
        m = build_model(model_id)
        out["models"][model_id] = {"sha256": layout_hash(m), "n_params": m.n_params, "shadow_t": m.shadow_t.numel(),
                                   "parameters": len(m.params)}
        print(model_id, out["models"][model_id])
    with open(os.path.join(HERE, "arena_layouts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
