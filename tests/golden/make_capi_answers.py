"""Generates tests/golden/capi_answers.json: what the host layer of libicamd.so (csrc/capi*.hip) answers without a GPU.

Run against the library of the commit whose answers are to be pinned -- the PARENT of a change to the C-ABI layer, built in a
worktree of its own, never the library under test (no GPU needed):
    python tests/golden/make_capi_answers.py --lib /path/to/parent/imageclassification_amd/csrc/libicamd.so

Two kinds of record, both pure host code:
  queries   every entry of hip._SIGNATURES whose name ends in _workspace_bytes, _supported or _stats_rows, over the argument lists
            of QUERY_ARGS (accepted and refused shapes; every query must give a nonzero answer at least once, checked here).
  refusals  every launching entry called once with all-zero arguments (NULL for every pointer and descriptor, 0 for every size):
            each must refuse before it reaches a HIP call, and the return code is recorded.  Such a call can never pass
            validation, so nothing is launched; the generator asserts every one returned nonzero.
  ordered   further refusals (ORDERED_REFUSALS) whose code depends on the ORDER of an entry's checks: every required pointer is
            given ("P": the address of a host buffer that is never read), and the shape is one the entry does not support, or the
            workspace size is 0 -- so the call ends in ICAMD_ERR_UNSUPPORTED or ICAMD_ERR_WORKSPACE (or ICAMD_ERR_BAD_ARG where a
            later check gives that).  Each is refused by a check that can be read off the entry; the generator asserts that the
            code is 1, 2 or 3, never 0 or ICAMD_ERR_LAUNCH.

The plans behind two size queries (the fused conv1x1 + BatchNorm backward and the stem weight gradient) read the CU count of the
device, which falls back to 256 when there is none -- the CU count of an MI355X, so the answers are the same with and without one.
tests/test_capi_answers_cpu.py reruns both against the built library and compares exactly.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QUERY_SUFFIXES = ("_workspace_bytes", "_supported", "_stats_rows")
# entries that neither answer a query nor launch: the ABI version, the profiler, the RCCL communicator bookkeeping, a pointer lookup
NOT_LAUNCHING = ("icamd_abi_version", "icamd_prof_enable", "icamd_prof_classes", "icamd_prof_collect", "icamd_rccl_available",
                 "icamd_rccl_version", "icamd_rccl_unique_id", "icamd_rccl_comm_init", "icamd_rccl_comm_info",
                 "icamd_rccl_comm_destroy", "icamd_image_pipeline_u8")

# descriptor id -> the eleven fields N, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad (None: a NULL descriptor)
DESCS = {
    "null": None,
    "pw_256_64_at_56": (32, 56, 56, 256, 56, 56, 64, 1, 1, 1, 0),        # bottleneck conv1: bnred / apply+conv fused
    "pw_64_256_at_56": (32, 56, 56, 64, 56, 56, 256, 1, 1, 1, 0),        # bottleneck conv3: fused conv3 + bn3 backward
    "pw_1024_256_at_14": (32, 14, 14, 1024, 14, 14, 256, 1, 1, 1, 0),
    "pw_s2_256_512": (32, 56, 56, 256, 28, 28, 512, 1, 1, 2, 0),         # projection shortcut
    "pw_small": (1, 8, 8, 64, 8, 8, 64, 1, 1, 1, 0),
    "pw_96_384": (8, 56, 56, 96, 56, 56, 384, 1, 1, 1, 0),               # ConvNeXt Mlp fc1
    "c3_64_at_56": (32, 56, 56, 64, 56, 56, 64, 3, 3, 1, 1),
    "c3_s2_128": (32, 56, 56, 128, 28, 28, 128, 3, 3, 2, 1),
    "c3_128_at_56": (32, 56, 56, 128, 56, 56, 128, 3, 3, 1, 1),          # grouped 3x3 with 32 groups
    "c3_odd": (3, 9, 11, 24, 9, 11, 40, 3, 3, 1, 1),
    "thin_32_32_at_112": (32, 112, 112, 32, 112, 112, 32, 3, 3, 1, 1),   # deep stem
    "thin_32_64_at_112": (32, 112, 112, 32, 112, 112, 64, 3, 3, 1, 1),
    "k7_s2_rgb": (2, 32, 32, 3, 16, 16, 16, 7, 7, 2, 3),
    "k4_s4_patch": (2, 56, 56, 3, 14, 14, 96, 4, 4, 4, 0),
    "bad_zero_batch": (0, 56, 56, 64, 56, 56, 64, 1, 1, 1, 0),
    "bad_output_size": (2, 56, 56, 64, 55, 56, 64, 1, 1, 1, 0),
    "bad_too_many_taps": (2, 32, 32, 64, 32, 32, 64, 9, 9, 1, 4),
}
_ALL = [[d] for d in DESCS]
_ROWS_C = [[0, 96], [394, 192], [100352, 96], [100352, 64], [100352, 256], [5, 7], [6272, 2048], [64, 4096], [64, 0]]
_NHWC = [[8, 56, 56, 96], [2, 7, 7, 768], [2, 14, 14, 384], [8, 56, 56, 100], [0, 56, 56, 96], [2, 12, 12, 768], [2, 7, 7, 96]]
_SE = [[32, 3136, 256], [2, 49, 2048], [0, 49, 64], [2, 49, 100], [3, 196, 1024], [2, 0, 64]]
_IMG = [[8, 500, 224, 224, 12], [2, 64, 32, 48, 4], [0, 500, 224, 224, 12], [8, 500, 224, 224, 0]]
# query -> argument lists; a string in first place is a descriptor id
QUERY_ARGS = {
    "icamd_conv2d_stats_rows": _ALL,
    "icamd_conv2d_dgrad_stats_rows": _ALL,
    "icamd_conv2d_dgrad_bnred_supported": _ALL,
    "icamd_bn_apply_conv1x1_fused_supported": _ALL,
    "icamd_conv1x1_bn_bwd_fused_supported": _ALL,
    "icamd_conv1x1_bn_bwd_fused_workspace_bytes": _ALL,
    "icamd_conv2d_wgrad_workspace_bytes": _ALL,
    "icamd_gconv3x3_supported": [[d, g] for d in DESCS for g in (32, 0, 3)],
    "icamd_gconv3x3_wgrad_workspace_bytes": [[d, g] for d in DESCS for g in (32, 0, 3)],
    "icamd_conv3x3_thin_supported": _ALL,
    "icamd_conv3x3_thin_stats_rows": _ALL,
    "icamd_conv3x3_thin_wgrad_workspace_bytes": _ALL,
    "icamd_bn_workspace_bytes": [[0], [-1], [64], [100], [2048], [4096]],
    "icamd_bn_bwd_workspace_bytes": _ROWS_C,
    "icamd_bn_bwd_apply_workspace_bytes": [[0], [-1], [64], [100], [2048], [4096]],
    "icamd_se_squeeze_workspace_bytes": _SE,
    "icamd_se_bn_bwd_workspace_bytes": _SE,
    "icamd_layernorm_bwd_workspace_bytes": _ROWS_C,
    "icamd_colsum_rows_workspace_bytes": _ROWS_C,
    "icamd_dwconv7_wgrad_workspace_bytes": _NHWC,
    "icamd_dwconv7_wgrad_bias_supported": _NHWC,
    "icamd_layerscale_bwd_workspace_bytes": _ROWS_C,
    # (Hs, Ws, window, D)
    "icamd_window_attention_supported": [[56, 56, 7, 32], [96, 96, 12, 32], [54, 54, 9, 32], [56, 56, 7, 64], [56, 56, 8, 32],
                                         [50, 56, 7, 32], [8, 8, 2, 32], [8, 8, 1, 32], [0, 0, 7, 32]],
    # (B, Hs, Ws, heads, window)
    "icamd_window_attention_bwd_workspace_bytes": [[2, 56, 56, 3, 7], [2, 96, 96, 4, 12], [2, 54, 54, 3, 9], [0, 56, 56, 3, 7],
                                                   [64, 56, 56, 3, 7], [64, 96, 96, 32, 12], [2, 56, 56, 0, 7], [1, 7, 7, 24, 7]],
    "icamd_patch_merge_ln_bwd_workspace_bytes": _NHWC,
    "icamd_stem7x7s2_stats_rows": [[32, 224, 224], [2, 64, 64], [1, 7, 8]],
    "icamd_stem7x7s2_wgrad_workspace_bytes": [[32, 224, 224, 64], [2, 64, 64, 64], [2, 64, 63, 64], [2, 64, 64, 60], [0, 64, 64, 64],
                                              [2, 6, 64, 64], [2, 64, 64, 32]],
    "icamd_image_pipeline_workspace_bytes": _IMG,
    "icamd_image_pipeline_aug_workspace_bytes": _IMG,
    "icamd_grad_norm_workspace_bytes": [[]],
}

P = "P"
# [entry, arguments]: "P" a non-NULL pointer, None NULL, a descriptor id in first place as in QUERY_ARGS
ORDERED_REFUSALS = [
    ["icamd_conv2d_dgrad", ["k7_s2_rgb", P, P, P, None, None, None]],                                  # Cin % 8 != 0
    ["icamd_conv2d_wgrad", ["pw_small", P, P, P, 0, P, 0, None]],                                      # workspace of 0 bytes
    ["icamd_conv2d_wgrad_bias", ["pw_small", P, P, P, P, 0, P, 0, None]],
    ["icamd_conv2d_dgrad_bnred", ["pw_small", P, P, P, P, None, 0, P, P, P, None]],                    # not a bnred shape
    ["icamd_gconv3x3_fwd", ["c3_128_at_56", 3, P, P, P, None, None]],                                  # 128 % 3 != 0
    ["icamd_gconv3x3_wgrad", ["c3_128_at_56", 32, P, P, P, 0, P, 0, None]],
    ["icamd_conv3x3_thin_fwd", ["c3_64_at_56", P, P, P, None, None, 0, None]],                         # Cin != 32
    ["icamd_conv3x3_thin_wgrad", ["thin_32_32_at_112", P, P, P, 0, P, 0, None]],
    ["icamd_bn_apply_conv1x1_fused", ["pw_small", P, P, P, P, None, None, P, P, P, P, None, None]],
    ["icamd_conv1x1_bn_bwd_fused", ["pw_small", None, 0, P, P, P, P, P, P, P, P, P, P, P, 0, P, 0, P, 0, None]],
    ["icamd_conv1x1_bn_bwd_fused", ["pw_64_256_at_56", None, 0, P, P, P, P, P, P, P, P, P, P, P, 0, P, 0, P, 0, None]],
    ["icamd_stem7x7s2_wgrad", [P, P, P, 0, P, 0, 2, 64, 63, 64, None]],                                # odd width: no size at all
    ["icamd_stem7x7s2_wgrad", [P, P, P, 0, P, 0, 2, 64, 64, 64, None]],
    ["icamd_bn_bwd", [P, None, P, P, P, P, P, P, P, P, None, None, 64, 8192, 0, 0, P, 0, None]],       # workspace before C > 4096
    ["icamd_bn_bwd_from_partials", [P, 1, P, P, P, P, P, P, P, P, 64, 64, 0, P, 0, None]],
    ["icamd_se_squeeze", [P, P, 2, 49, 100, P, 0, None]],                                              # shape before workspace
    ["icamd_se_squeeze", [P, P, 2, 49, 2048, P, 0, None]],
    ["icamd_layernorm_bwd", [P, P, P, P, P, None, P, P, P, 394, 192, 0, P, 0, None]],
    ["icamd_colsum_rows", [P, 394, 192, 192, P, 0, P, 0, None]],
    ["icamd_dwconv7_wgrad", [P, P, P, 0, P, 0, 8, 56, 56, 100, None]],                                 # C % 32 != 0
    ["icamd_layerscale_bwd", [P, P, P, None, P, P, 394, 192, 197, 0, P, 0, None]],
    ["icamd_rows_fix", [P, 2, P, P, 8, None, 0, None]],                                                # bytes % 16 != 0
    ["icamd_attention_fwd", [P, P, P, 1, 1, 1, 32, 1.0, None]],                                        # D != 64
    ["icamd_window_attention_fwd", [P, P, P, P, 2, 54, 54, 3, 32, 9, 0, 1.0, None]],                   # window 9
    ["icamd_window_attention_fwd", [P, P, P, P, 2, 56, 56, 3, 32, 7, 7, 1.0, None]],                   # shift >= window
    ["icamd_window_attention_bwd", [P, P, P, P, P, P, P, 0, P, 0, 2, 56, 56, 3, 32, 7, 0, 1.0, None]],
    ["icamd_relpos_bias_gather", [P, P, 3, 9, None]],
    ["icamd_patch_merge_ln_fwd", [P, P, P, P, P, P, 2, 7, 7, 96, 1e-5, None]],                         # odd side
    ["icamd_patch_merge_ln_bwd", [P, P, P, P, P, P, P, P, 2, 56, 56, 96, 0, P, 0, None]],
    ["icamd_pack_input", [P, P, 3, 3, 8, 8, 1, 0.5, 0, 0, 0, 0, None]],                                # mixing needs an even batch
    ["icamd_image_pipeline", [P, P, 2, 64, 32, 48, 0, 4, P, P, P, P, 0, None]],
]
_HOST = ctypes.create_string_buffer(4096)      # what "P" points to


def bind(path):
    """The library at `path` with the signatures of hip._SIGNATURES (hip.load() binds only the package's own copy)."""
    from imageclassification_amd import hip
    lib = ctypes.CDLL(path)
    for name, (res, args) in hip._SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def query_names():
    from imageclassification_amd import hip
    return [n for n in hip._SIGNATURES if n.endswith(QUERY_SUFFIXES)]


def launching_names():
    from imageclassification_amd import hip
    return [n for n in hip._SIGNATURES if not n.endswith(QUERY_SUFFIXES) and n not in NOT_LAUNCHING]


def ask(lib, name, args):
    """One call; a leading descriptor id becomes a pointer to that descriptor (NULL for "null"), "P" a pointer to _HOST."""
    from imageclassification_amd import hip
    args = list(args)
    if args and isinstance(args[0], str) and args[0] != P:
        fields = DESCS[args[0]]
        args[0] = None if fields is None else ctypes.byref(hip.ConvDesc(*fields))
    for k, t in enumerate(hip._SIGNATURES[name][1]):
        if args[k] == P:
            args[k] = ctypes.addressof(_HOST) if t is ctypes.c_void_p else ctypes.cast(_HOST, t)
    return int(getattr(lib, name)(*args))


def refuse(lib, name):
    """The return code of `name` called with NULL for every pointer and 0 for everything else."""
    from imageclassification_amd import hip
    zeros = [None if (t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)) else t(0) for t in hip._SIGNATURES[name][1]]
    return int(getattr(lib, name)(*zeros))


def answers(lib):
    """{"queries": {name: [[arguments, answer], ...]}, "refusals": {name: return code}, "ordered": [[name, arguments, return code], ...]}"""
    return {"queries": {n: [[a, ask(lib, n, a)] for a in QUERY_ARGS[n]] for n in query_names()},
            "refusals": {n: refuse(lib, n) for n in launching_names()},
            "ordered": [[n, a, ask(lib, n, a)] for n, a in ORDERED_REFUSALS]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libicamd.so of the commit whose answers are pinned (the parent's build)")
    a = ap.parse_args()
    assert sorted(QUERY_ARGS) == sorted(query_names()), set(QUERY_ARGS) ^ set(query_names())
    got = answers(bind(os.path.abspath(a.lib)))
    for n, rows in got["queries"].items():
        assert any(v != 0 for _, v in rows), f"{n}: every answer is zero"
        print(n, sum(1 for _, v in rows if v != 0), "of", len(rows), "nonzero")
    for n, rc in got["refusals"].items():
        assert rc != 0, f"{n} accepted all-zero arguments"
    for n, a, rc in got["ordered"]:
        assert rc in (1, 2, 3), f"{n}{a} returned {rc}"
    print(len(got["queries"]), "queries,", len(got["refusals"]), "refusals,", len(got["ordered"]), "ordered refusals")
    with open(os.path.join(HERE, "capi_answers.json"), "w") as f:      # one query per line
        f.write('{\n "generator": "tests/golden/make_capi_answers.py",\n "queries": {\n')
        f.write(",\n".join(f'  "{n}": {json.dumps(rows)}' for n, rows in got["queries"].items()))
        f.write('\n },\n "refusals": ' + json.dumps(got["refusals"], indent=2).replace("\n", "\n ") + ',\n "ordered": [\n')
        f.write(",\n".join("  " + json.dumps(r) for r in got["ordered"]) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
