"""Shared by the window-12 Swin tests: the two new configurations beside a copy of the reference's own table, reference models
built from that copy, and Python mirrors of the launch planner of csrc/window_attention_w12.hip (each names the C++ function it
restates).  Nothing here touches a GPU."""
import contextlib

import torch

import _swin_ref as SR

T12 = 144

# a copy of tests/_swin_ref.py's table with the window-12 configurations: (embed dim, depths, heads, window)
CONFIGS = dict(SR.CONFIGS)
CONFIGS["swin_base_patch4_window12_384"] = (128, (2, 2, 18, 2), (4, 8, 16, 32), 12)
CONFIGS["swin_test_w12"] = (32, (2, 2), (1, 2), 12)


@contextlib.contextmanager
def _extended_table():
    """SwinRef looks names up in its module's table: show it the extended copy while a model is built"""
    saved = SR.CONFIGS
    SR.CONFIGS = CONFIGS
    try:
        yield
    finally:
        SR.CONFIGS = saved


def swin_ref(arch, num_classes, img_size, bf16_points=False):
    with _extended_table():
        return SR.SwinRef(arch, num_classes, img_size=img_size, bf16_points=bf16_points)


def perturbed_ref(arch, C, img, seed=0):
    """the reference with bf16 rounding points and non-trivial biases, LayerNorm affine and bias tables"""
    torch.manual_seed(seed)
    ref = swin_ref(arch, C, img, bf16_points=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("relative_position_bias_table"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "norm" in n and n.endswith("weight"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
    return ref


def pair(arch, C, img, seed=0, drop_path_rate=0.0):
    """tests/test_swin_gpu.py _pair with the extended table: the reference with non-trivial biases, LayerNorm affine and bias tables,
    and the model under test loaded from its state_dict"""
    from imageclassification_amd.swin import SwinTransformer
    ref = perturbed_ref(arch, C, img, seed)
    net = SwinTransformer(arch, C, img_size=img, drop_path_rate=drop_path_rate)
    net.load_state_dict(ref.state_dict())
    return ref, net


# ---------------------------------------------------------------------------------------------------------------- planners
FWD_CAP, BWD_CAP = 2048, 512     # workgroups of a launch, all heads together (csrc/window_attention_w12.hip)


def chunks12(nwin, H, cap):
    """chunks12 (csrc/window_attention_w12.hip): workgroups per head, one window per workgroup and trip"""
    return min(nwin, max(cap // H, 1))


def fwd_grid(nwin, H):
    """icamd_window_attention_w12_fwd_launch: workgroups per head"""
    return chunks12(nwin, H, FWD_CAP)


def bwd_grid(nwin, H):
    """icamd_window_attention_w12_bwd_chunks: workgroups = dbias partials per head"""
    return chunks12(nwin, H, BWD_CAP)


def trips(nwin, grid):
    """trips of the window loop of winattn12_fwd_kernel / winattn12_bwd_kernel (wi = block + trip * grid) for the busiest workgroup"""
    return (nwin + grid - 1) // grid


def bwd_workspace_bytes(B, Hs, Ws, H):
    """icamd_window_attention_bwd_workspace_bytes for ws = 12"""
    nwin = B * (Hs // 12) * (Ws // 12)
    return (bwd_grid(nwin, H) * H * T12 * T12 * 4 + 255) // 256 * 256
