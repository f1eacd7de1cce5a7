"""Every in-tree kernel instance the benchmark steps launch (the r05 kernel-trace profiles of the four headline runs) is
launched at full size by tests/test_fullsize_layers_gpu.py (the per-layer kernels) or tests/test_fullsize_step_gpu.py (loss,
metrics, optimizer, EMA, input packing, filter preparation) -- their own kernel-trace profiles,
profiles/fullsize_layers_kernel_stats.csv and profiles/fullsize_step_kernel_stats.csv -- so each of them is compared element
by element at the grids the benchmark produces.  An instance is the kernel with its template arguments; the parameter list
is dropped.  No kernel is let off."""
import csv
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ["r05_bench_n1_kernel_stats_single_stream.csv", "r05_eval_kernel_stats.csv", "r05_vit_b16_kernel_stats.csv",
            "r05_convnext_t_mixup_ema_kernel_stats.csv"]
FULLSIZE = ["fullsize_layers_kernel_stats.csv", "fullsize_step_kernel_stats.csv"]
STEP_GRIDS = "fullsize_step_kernel_grids.csv"     # per kernel and grid of the step module's trace: workgroups, launches

# the step module's own profile must hold the kernels every step ends in -- and the optimizers and the gradient guard that
# only --opt / --update_freq launch, which no benchmark profile lists
STEP_KERNELS = ["adamw_ema_kernel", "lerp_kernel", "sumsq_partial_kernel", "gradnorm_finalize_kernel", "f32_to_bf16_kernel",
                "filter_transpose_kernel", "filter_transpose_tiled_kernel", "bn_fold_kernel", "layerscale_fold_kernel",
                "softmax_xent_kernel", "step_metrics_kernel", "pack_input_kernel", "pack_input_rgb4_kernel",
                "optim_ema_kernel<1>", "optim_ema_kernel<2>", "optim_ema_kernel<3>", "optim_ema_kernel<4>", "grad_guard_kernel"]


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
    covered = set().union(*(instances(f) for f in FULLSIZE))
    missing = {}
    for fname in PROFILES:
        for inst in instances(fname):
            if inst.startswith("at::native") or inst.startswith("__amd_rocclr_") or base(inst) not in tree:
                continue
            if inst in covered:
                continue
            missing.setdefault(inst, fname)
    assert not missing, "launched by the benchmark, never at full size by the layer or step tests:\n" + "\n".join(
        f"  {k}  ({v})" for k, v in sorted(missing.items()))


def test_step_profile_holds_the_step_kernels_at_their_capped_grids():
    tree = in_tree_kernels()
    assert {base(k) for k in STEP_KERNELS} <= tree, sorted({base(k) for k in STEP_KERNELS} - tree)
    step = instances(FULLSIZE[1])
    assert set(STEP_KERNELS) <= step, sorted(set(STEP_KERNELS) - step)
    with open(os.path.join(ROOT, "profiles", STEP_GRIDS), newline="") as f:
        rows = [(instance(r["Name"]), int(r["Workgroups"]), int(r["Workgroup_Size"])) for r in csv.DictReader(f)]
    assert {n for n, _, _ in rows} == {i for i in step if base(i) in tree}
    grids = {}
    for n, g, _ in rows:
        grids.setdefault(n, set()).add(g)
    # the grid-stride kernels ran at their caps (so their loops took several trips): 2048 workgroups, 512 for the norm
    for k in ["adamw_ema_kernel", "optim_ema_kernel<1>", "optim_ema_kernel<2>", "optim_ema_kernel<3>", "optim_ema_kernel<4>",
              "grad_guard_kernel", "lerp_kernel", "f32_to_bf16_kernel", "pack_input_kernel", "pack_input_rgb4_kernel"]:
        assert max(grids[k]) == 2048, (k, grids[k])
    assert grids["sumsq_partial_kernel"] == {512} and grids["gradnorm_finalize_kernel"] == {1}
    assert max(grids["softmax_xent_kernel"]) == 96 and grids["step_metrics_kernel"] == {1}
    assert all(w in (64, 256) for _, _, w in rows)
