"""Shared by the tests of the small ConvNeXt models (widths that are no multiple of 32): the family table and its parameter counts,
the registration of the narrow V2 names with the package for the length of a test, Python mirrors of the depthwise weight-gradient
geometry and of the GRN launch planner, and the GRN entries on tensors.

Importing this module needs no GPU and makes no CUDA call."""
import contextlib

import torch

from oracle.convnext_ref import GRN_EPS

# name stem -> (depths, dims, V1 parameters at 1000 classes or None, V2 parameters or None)
FAMILY = {
    "atto": ((2, 2, 6, 2), (40, 80, 160, 320), 3695520, 3708400),
    "femto": ((2, 2, 6, 2), (48, 96, 192, 384), 5217784, 5233240),
    "pico": ((2, 2, 6, 2), (64, 128, 256, 512), 9045672, 9066280),
    "nano": ((2, 2, 8, 2), (80, 160, 320, 640), 15593560, 15623800),
    "tiny": ((3, 3, 9, 3), (96, 192, 384, 768), 28589128, 28635496),
    "small": ((3, 3, 27, 3), (96, 192, 384, 768), None, None),
    "base": ((3, 3, 27, 3), (128, 256, 512, 1024), 88591464, 88717800),
    "large": ((3, 3, 27, 3), (192, 384, 768, 1536), 197767336, 197956840),
}

NARROW = ((1, 1, 2, 1), (40, 80, 160, 320))


def param_count(depths, dims, v2, num_classes=1000):
    """stem 4x4 conv + LN; per stage LN + 2x2 conv; per block dw 7x7, LN, fc1, fc2 and gamma (V1) or GRN weight + bias (V2);
    head norm + fc"""
    n = (3 * 16 * dims[0] + dims[0]) + 2 * dims[0]
    for i, (depth, d) in enumerate(zip(depths, dims)):
        if i:
            p = dims[i - 1]
            n += 2 * p + (p * 4 * d + d)
        block = (49 * d + d) + 2 * d + (d * 4 * d + 4 * d) + (4 * d * d + d) + (8 * d if v2 else d)
        n += depth * block
    return n + 2 * dims[-1] + dims[-1] * num_classes + num_classes


V2_UNREGISTERED = {"convnextv2_atto": FAMILY["atto"][:2], "convnextv2_femto": FAMILY["femto"][:2],
                   "convnextv2_nano": FAMILY["nano"][:2], "convnextv2_test_narrow": NARROW}


@contextlib.contextmanager
def narrow_registered():
    """For the length of a `with`: the V2 models of narrow widths in convnext.CONFIGS / GRN_ARCHS.  The class and the kernels run
    those, but the package does not list them (tests/test_convnextv2_cpu.py pins its V2 names to the oracle's), so the tests that
    drive the V2 block at these widths add them here.  Everything is taken out again: other test modules compare these tables.
    (The oracle needs no registration: it builds any (depths, dims) pair.)"""
    from imageclassification_amd import convnext
    grn = convnext.GRN_ARCHS
    convnext.CONFIGS.update(V2_UNREGISTERED)
    convnext.GRN_ARCHS = grn | set(V2_UNREGISTERED)
    try:
        yield
    finally:
        for name in V2_UNREGISTERED:
            del convnext.CONFIGS[name]
        convnext.GRN_ARCHS = grn


def cdiv(a, b):
    return (a + b - 1) // b


def dw_wgrad_geometry(N, H, W, C):
    """dw_wgrad_rows_geometry (csrc/dwconv.hip) for C % 32 != 0, and the trips of the problem-sized loops of
    dwconv7_wgrad_runs_kernel / dw_wgrad_pass for the busiest thread"""
    assert C % 8 == 0 and C % 32 != 0
    cpr = C // 2
    slice_ = min(cpr, 256)
    while cpr % slice_:
        slice_ -= 1
    groups, nslices, nstrips = 256 // slice_, cpr // slice_, cdiv(W, 7)
    iblocks = cdiv(N * nstrips, groups)
    return {"slice": slice_, "groups": groups, "idle": 256 - groups * slice_, "nslices": nslices, "nstrips": nstrips,
            "iblocks": iblocks, "workspace": iblocks * 50 * C * 4,
            "trips": {"rows, first pass (base += 4)": cdiv(H, 4), "rows, second pass (base += 3)": cdiv(H, 3),
                      "lds outputs (idx += 256)": cdiv(14 * slice_, 256), "groups summed": groups,
                      "bias lds outputs": cdiv(2 * slice_, 256), "slab rows folded": iblocks}}


def grn_plan(N, HW, C):
    """icamd_grn_plan and reduce_tcols (csrc/grn.hip), and the trip count of every loop of its kernels whose length depends on
    the problem, for the busiest thread."""
    cpr = C // 8
    S = max(min(cdiv(2048, N), cdiv(HW, 32), 64), 1)
    rps = cdiv(HW, S)
    S = cdiv(HW, rps)
    B = max(min(cdiv(HW * cpr, 1024), cdiv(4096, N), cdiv(HW, 8)), 1)
    rpb = cdiv(HW, B)
    B = cdiv(HW, rpb)
    tcols = cpr if cpr <= 256 else max(t for t in range(8, 257, 8) if cpr % t == 0)
    rlanes = 256 // tcols
    return {"S": S, "rps": rps, "B": B, "rpb": rpb, "tcols": tcols, "ctiles": cpr // tcols, "rlanes": rlanes,
            "trips": {"reduce rows": cdiv(rps, rlanes),                  # grn_reduce_kernel: r += rlanes
                      "reduce lds outputs": cdiv(tcols * 8, 256),        # o += 256 (the backward's walks twice as far)
                      "reduce row lanes": rlanes,                        # l < rlanes
                      "prologue channels": cdiv(C, 1024),                # c4 += 256, four channels each (grn_stats, s / t loops)
                      "prologue segments": S,                            # s < S
                      "apply vectors": cdiv(rpb * cpr, 256),             # i += 256
                      "parameter-gradient samples": cdiv(N, 4)}}         # grn_param_grads_kernel: n += 4


class Grn:
    """icamd_grn_fwd / icamd_grn_bwd on tensors"""

    def __init__(self, N, HW, C):
        from imageclassification_amd import hip
        self.hip, self.lib = hip, hip.load()
        self.N, self.HW, self.C = N, HW, C
        self.bytes = self.lib.icamd_grn_workspace_bytes(N, HW, C)
        self.ws = torch.empty(max(self.bytes, 256), dtype=torch.uint8, device="cuda")

    def fwd(self, a, gamma, beta):
        g, gx = torch.empty_like(a), torch.empty(self.N, self.C, device="cuda")
        rc = self.lib.icamd_grn_fwd(a.data_ptr(), gamma.data_ptr(), beta.data_ptr(), g.data_ptr(), gx.data_ptr(), self.N, self.HW,
                                    self.C, GRN_EPS, self.ws.data_ptr(), self.bytes, self.hip.stream_ptr())
        return rc, g, gx

    def bwd(self, dg, a, gx, gamma, z=None, dgamma=None, dbeta=None, accumulate=0):
        dx = torch.empty_like(a)
        dgamma = torch.empty(self.C, device="cuda") if dgamma is None else dgamma
        dbeta = torch.empty(self.C, device="cuda") if dbeta is None else dbeta
        rc = self.lib.icamd_grn_bwd(dg.data_ptr(), a.data_ptr(), gx.data_ptr(), gamma.data_ptr(), None if z is None else z.data_ptr(),
                                    dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), accumulate, self.N, self.HW, self.C,
                                    GRN_EPS, self.ws.data_ptr(), self.bytes, self.hip.stream_ptr())
        return rc, dx, dgamma, dbeta
