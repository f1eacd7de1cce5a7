"""Shared by the window-12 Swin tests: Python mirrors of the launch planner of csrc/window_attention_w12.hip (each names the C++
function it restates).  Nothing here touches a GPU."""
T12 = 144

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
