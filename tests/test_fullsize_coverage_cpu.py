"""Every in-tree kernel instance the benchmark steps launch (the r05 kernel-trace profiles of the four headline runs) is
launched by tests/test_fullsize_layers_gpu.py at full size (its own kernel-trace profile,
profiles/fullsize_layers_kernel_stats.csv) -- so each of them is compared element by element at the grids the benchmark
produces.  An instance is the kernel with its template arguments; the parameter list is dropped.  Only kernels whose work
does not scale with the batch layer by layer may be left out, each with its reason below."""
import csv
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ["r05_bench_n1_kernel_stats_single_stream.csv", "r05_eval_kernel_stats.csv", "r05_vit_b16_kernel_stats.csv",
            "r05_convnext_t_mixup_ema_kernel_stats.csv"]
FULLSIZE = "fullsize_layers_kernel_stats.csv"

EXCEPTIONS = {
    "adamw_ema_kernel": "optimizer step + EMA: one pass over the parameters",
    "lerp_kernel": "EMA lerp over the parameters",
    "sumsq_partial_kernel": "gradient-norm partial sums over the parameters",
    "gradnorm_finalize_kernel": "gradient-norm finalize: one vector",
    "f32_to_bf16_kernel": "bf16 shadow of the fp32 parameters (optimizer side)",
    "filter_transpose_kernel": "filter transpose for the data gradient",
    "filter_transpose_tiled_kernel": "filter transpose for the data gradient",
    "bn_fold_kernel": "eval BatchNorm fold into the filters",
    "layerscale_fold_kernel": "layer-scale fold into the fc2 filter",
    "softmax_xent_kernel": "loss over the logits",
    "step_metrics_kernel": "loss / accuracy metrics",
    "pack_input_kernel": "input packing",
    "pack_input_rgb4_kernel": "input packing",
}


def instance(name):
    """Kernel name without its return type and parameter list, template arguments kept."""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += {")": 1, "(": -1}.get(name[i], 0)
            if depth == 0:
                name = name[:i]
                break
    return name.replace("(anonymous namespace)::", "").strip()


def base(inst):
    return inst.split("<", 1)[0].split("::")[-1]


def in_tree_kernels():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "imageclassification_amd", "csrc", "*.hip")):
        src = open(path).read()
        for m in re.finditer(r"__global__", src):
            head = re.sub(r"__launch_bounds__\s*\([^)]*\)", "", src[m.end():m.end() + 400])
            names.add(re.match(r"[^(]*?(\w+)\s*\(", head).group(1))
    return names


def instances(fname):
    with open(os.path.join(ROOT, "profiles", fname), newline="") as f:
        return {instance(r["Name"]) for r in csv.DictReader(f)}


def test_instance_names():
    assert instance("void (anonymous namespace)::conv_igemm_kernel<128, 0, 2>(IgemmParams)") == "conv_igemm_kernel<128, 0, 2>"
    assert instance("(anonymous namespace)::bn_apply_kernel(unsigned short const*, float const*, long long)") == "bn_apply_kernel"
    assert base("conv_wgrad_ring_kernel<256, 128, 2, 2, 3, 2>") == "conv_wgrad_ring_kernel"


def test_every_benchmark_kernel_instance_is_compared_at_full_size():
    tree = in_tree_kernels()
    assert {"conv_igemm_kernel", "attn_fwd_kernel", "bn_reduce_finalize_kernel"} <= tree
    assert set(EXCEPTIONS) <= tree, sorted(set(EXCEPTIONS) - tree)
    covered = instances(FULLSIZE)
    missing = {}
    for fname in PROFILES:
        for inst in instances(fname):
            if inst.startswith("at::native") or inst.startswith("__amd_rocclr_") or base(inst) not in tree:
                continue
            if base(inst) in EXCEPTIONS or inst in covered:
                continue
            missing.setdefault(inst, fname)
    assert not missing, "launched by the benchmark, never at full size by the layer tests:\n" + "\n".join(
        f"  {k}  ({v})" for k, v in sorted(missing.items()))
