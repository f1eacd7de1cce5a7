"""csrc/workspace.h without a GPU: the one layout function of each multi-region workspace, which both the size query and the
carve go through.  tests/workspace_layout_main.cpp is built with the host compiler under AddressSanitizer + UBSan and run once as
a child process over the grid below: per case it allocates exactly `bytes` bytes, carves them and writes every region, so a total
that falls short of its carve is a sanitizer report, and it prints the offsets.  Those are compared with the arithmetic of the
commit BEFORE the header existed, restated here by hand from that commit's entries (capi_norm.hip, capi_tokens.hip, se_ops.hip,
grn.hip, image_ops.hip, capi.hip), not from workspace.h; the totals are compared with the built library's size queries."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "imageclassification_amd", "csrc")
AUG_AUX_BYTES = 768 + 16          # image_ops.hip: a 3 x 256 LUT and 16 B more per image


def up(v):
    return (v + 255) // 256 * 256


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the layouts as the entries carved them by hand: name -> ([(offset, bytes the kernels touch), ...], total) ---------------------
def reduce_ref(C, rows, k):
    chunk = 256 + up(64 * 2 * C * 8)                      # bn_chunk_bytes: counters, then [64][2][C] doubles
    scratch = chunk + up(rows * 2 * C * 4)
    return [(0, 256), (256, 64 * 2 * C * 8), (chunk, rows * 2 * C * 4), (scratch, k * C * 4)], scratch + up(k * C * 4)


def se_ref(N, S, C):
    nc = up(N * C * 4)
    ab = up(N * S * 2 * C * 4)
    dh = ab + 5 * nc
    k2 = dh + up(N * 256 * 4)
    return [(0, N * S * 2 * C * 4), (ab, 2 * N * C * 4), (ab + 2 * nc, N * C * 4), (ab + 3 * nc, N * C * 4), (ab + 4 * nc, N * C * 4),
            (dh, N * 256 * 4), (k2, C * 4)], k2 + up(C * 4)


def grn_ref(N, S, C):
    fin = up(N * S * 2 * C * 4)
    return [(0, N * S * 2 * C * 4), (fin, N * 2 * C * 4)], fin + up(N * 2 * C * 4)


def image_ref(B, tab_words, mch, oh, ow):
    tabs_b, tmp_b = up(B * tab_words * 4), up(B * mch * ow * 3)
    return [(0, B * tab_words * 4), (tabs_b, B * mch * ow * 3), (tabs_b + tmp_b, B * oh * ow * 3)], tabs_b + tmp_b + up(B * oh * ow * 3)


def image_aug_ref(B, tab_words, mch, oh, ow, aux):
    regions, base = image_ref(B, tab_words, mch, oh, ow)
    img_b = up(B * oh * ow * 3)
    return regions + [(base, B * oh * ow * 3), (base + img_b, B * aux)], base + img_b + up(B * aux)


def wgrad_ref(S, Cout, Ktot):
    return [(0, S * Cout * Ktot * 4), (S * Cout * Ktot * 4, S * Cout * 4)], S * Cout * (Ktot + 1) * 4


REF = {"reduce": reduce_ref, "se": se_ref, "grn": grn_ref, "image": image_ref, "image_aug": image_aug_ref, "wgrad": wgrad_ref}
# Regions start 256 B aligned, but for the one the entries never rounded: the bias rows follow the filter slabs directly (fp32).
ALIGN = {"wgrad": 4}


# ---- the plans behind the size queries (norm_pool.hip, token_ops.hip, dwconv.hip, se_ops.hip, grn.hip, image_ops.hip) ----------------
def bn_bwd_blocks(rows):
    return cdiv(rows, max(cdiv(rows, 1024), 32))


def layernorm_bwd_blocks(rows):
    return (min(rows, 4096) + 3) // 4


colsum_blocks = layerscale_bwd_blocks = bn_bwd_blocks     # the same two lines in each of the three units


def se_segments(N, HW):
    s = max(min(cdiv(2048, N), cdiv(HW, 32)), 1)
    return cdiv(HW, cdiv(HW, s))


def grn_segments(N, HW):
    s = max(min(cdiv(2048, N), cdiv(HW, 32), 64), 1)
    return cdiv(HW, cdiv(HW, s))


def tab_words(oh, ow, kmax):
    return (oh + ow) * (2 + kmax)


# ---- the grid: smallest cases, sizes off the 256 B grain, no partial rows / no scratch rows -----------------------------------------
GRID = [("reduce", C, rows, k) for C in (7, 8, 64, 100, 192, 4096) for rows in (0, 1, 3, 99) for k in (0, 2, 3)]
GRID += [("se", N, S, C) for N in (1, 2, 3, 32) for S in (1, 2, 7) for C in (8, 64, 104, 4096)]
GRID += [("grn", N, S, C) for N in (1, 3, 8) for S in (1, 5, 64) for C in (128, 192, 6144)]
_IMAGES = [(1, 6, 1, 1, 1), (3, 77, 5, 7, 9), (2, tab_words(32, 48, 4), 64, 32, 48), (8, tab_words(224, 224, 12), 500, 224, 224)]
GRID += [("image",) + i for i in _IMAGES] + [("image_aug",) + i + (aux,) for i in _IMAGES for aux in (AUG_AUX_BYTES, 5)]
GRID += [("wgrad", S, Cout, Ktot) for S, Cout, Ktot in ((1, 8, 8), (1, 64, 64), (7, 1, 1), (3, 40, 216), (2, 256, 576), (5, 96, 48))]


def _library_cases():
    """(query, arguments, layout case) for every accepted shape of tests/golden/capi_answers.json whose query sizes one of the
    layouts, with the block count of the plan restated above."""
    with open(os.path.join(HERE, "golden", "capi_answers.json")) as f:
        queries = json.load(f)["queries"]
    out = []

    def accepted(name):
        return [a for a, v in queries[name] if v != 0]

    out += [("icamd_bn_workspace_bytes", a, ("reduce", a[0], 0, 0)) for a in accepted("icamd_bn_workspace_bytes")]
    out += [("icamd_bn_bwd_apply_workspace_bytes", a, ("reduce", a[0], 0, 2)) for a in accepted("icamd_bn_bwd_apply_workspace_bytes")]
    for name, blocks, k in (("icamd_bn_bwd_workspace_bytes", bn_bwd_blocks, 2), ("icamd_layernorm_bwd_workspace_bytes", layernorm_bwd_blocks, 2),
                            ("icamd_colsum_rows_workspace_bytes", colsum_blocks, 3), ("icamd_layerscale_bwd_workspace_bytes", layerscale_bwd_blocks, 3)):
        out += [(name, a, ("reduce", a[1], blocks(a[0]), k)) for a in accepted(name)]
    out += [("icamd_se_bn_bwd_workspace_bytes", a, ("se", a[0], se_segments(a[0], a[1]), a[2])) for a in accepted("icamd_se_bn_bwd_workspace_bytes")]
    out += [("icamd_image_pipeline_workspace_bytes", a, ("image", a[0], tab_words(a[2], a[3], a[4]), a[1], a[2], a[3]))
            for a in accepted("icamd_image_pipeline_workspace_bytes")]
    out += [("icamd_image_pipeline_aug_workspace_bytes", a, ("image_aug", a[0], tab_words(a[2], a[3], a[4]), a[1], a[2], a[3], AUG_AUX_BYTES))
            for a in accepted("icamd_image_pipeline_aug_workspace_bytes")]
    # global response normalisation arrived after that record: (N, rows per image, C) of the ConvNeXt V2 test and atto models
    out += [("icamd_grn_workspace_bytes", list(a), ("grn", a[0], grn_segments(a[0], a[1]), a[2]))
            for a in ((8, 256, 128), (1, 1, 128), (3, 49, 1280), (64, 3136, 320), (2, 100, 6144))]
    return out


LIBRARY_CASES = _library_cases()


def _compiler():
    """$CXX, else c++, else the clang++ of the ROCm install that builds the library."""
    for c in (os.environ.get("CXX"), "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")):
        if os.path.exists(c):
            return c
    raise AssertionError("no host C++ compiler: neither $CXX, c++ nor the ROCm clang++")


@pytest.fixture(scope="module")
def carved(tmp_path_factory):
    """{case: (bytes, [offsets])} from ONE run of the sanitized program over the grid and the library's shapes."""
    exe = str(tmp_path_factory.mktemp("workspace_layout") / "workspace_layout_main")
    subprocess.run([_compiler(), "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1",
                    os.path.join(HERE, "workspace_layout_main.cpp"), "-o", exe], check=True)
    cases = list(dict.fromkeys(GRID + [c for _, _, c in LIBRARY_CASES]))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")     # every block is freed; the leak pass needs ptrace, which a sandbox may deny
    run = subprocess.run([exe], input="".join(" ".join(map(str, c)) + "\n" for c in cases), capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    out = {}
    for case, line in zip(cases, lines):
        kind, *nums = line.split()
        assert kind == case[0]
        out[case] = (int(nums[0]), [int(v) for v in nums[1:]])
    return out


@pytest.mark.parametrize("kind", list(REF))
def test_offsets_and_totals_are_the_hand_carved_ones(carved, kind):
    cases = [c for c in carved if c[0] == kind]
    assert len(cases) >= 4
    for case in cases:
        regions, total = REF[kind](*case[1:])
        nbytes, offsets = carved[case]
        assert offsets == [o for o, _ in regions] and nbytes == total, case
        assert all(o % ALIGN.get(kind, 256) == 0 for o in offsets), case
        ends = [o + n for o, n in regions]
        assert all(e <= o for e, o in zip(ends, offsets[1:])) and ends[-1] <= nbytes, case       # in order, disjoint, inside


def test_totals_are_the_librarys_answers(carved):
    from imageclassification_amd import hip
    lib = hip.load()
    assert {n for n, _, _ in LIBRARY_CASES} >= {"icamd_bn_workspace_bytes", "icamd_bn_bwd_workspace_bytes", "icamd_se_bn_bwd_workspace_bytes",
                                                "icamd_image_pipeline_aug_workspace_bytes", "icamd_grn_workspace_bytes"}
    for name, args, case in LIBRARY_CASES:
        assert int(getattr(lib, name)(*args)) == carved[case][0] != 0, (name, args)


def test_weight_gradient_total_is_the_librarys_answer():
    """The split count S of the dense weight gradient comes from a cost model that is not restated here, and no query publishes
    it: every recorded answer is a whole number S of [Cout][Ktot + 1] fp32 slabs, and the hand layout at that S gives it back."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_capi_answers", os.path.join(HERE, "golden", "make_capi_answers.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    from imageclassification_amd import hip
    lib = hip.load()
    seen = 0
    for desc, fields in G.DESCS.items():
        answer = G.ask(lib, "icamd_conv2d_wgrad_workspace_bytes", [desc])
        if answer == 0:
            continue
        _, _, _, Cin, _, _, Cout, KH, KW, _, _ = fields
        slab = Cout * (KH * KW * Cin + 1) * 4
        assert answer % slab == 0, desc
        assert wgrad_ref(answer // slab, Cout, KH * KW * Cin)[1] == answer
        seen += 1
    assert seen >= 10


def test_no_hand_carving_left_in_csrc():
    """No `ws +=` walk and no inline round-up to 256 outside workspace.h."""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name == "workspace.h" or not name.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            for i, line in enumerate(f, 1):
                if re.search(r"\bws\s*\+=|/\s*256\s*\*\s*256", line):
                    hits.append(f"{name}:{i}: {line.strip()}")
    assert hits == []
