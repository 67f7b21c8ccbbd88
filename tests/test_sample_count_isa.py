"""Resources of the render kernels that S != 64 samples per ray launch (csrc/render.hip, rgb_fwd.hip, rgb_bwd.hip: the GEN / _ns
instances), against the S = 64 instance of the same variant, from the code objects hipcc cross-compiles without a GPU; and the host
test of the supported family."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shapeclipper_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _kernels(asm):
    """{kernel symbol: (private_segment_fixed_size, vgpr_spill_count, vgpr_count)} from the amdhsa metadata of an assembly listing."""
    out = {}
    for block in re.split(r"\n\s+- \.", asm):
        name = re.search(r"^\s*\.?name:\s+(\S+)", block, flags=re.M)
        priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
        if name and priv and spill and vgpr and "kernel" in name.group(1):
            out[name.group(1)] = (int(priv.group(1)), int(spill.group(1)), int(vgpr.group(1)))
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tmp_path_factory.mktemp("isa")

    def build(name):
        out = str(tmp / (name + ".s"))
        extra = ["-ffp-contract=off"] if name == "render" else []
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-I" + os.path.join(ROOT, "include"),
                            *extra, "-S", "--cuda-device-only", os.path.join(CSRC, name + ".hip"), "-o", out],
                           capture_output=True, text=True, cwd=CSRC)
        assert r.returncode == 0, r.stderr[-2000:]
        return _kernels(open(out).read())
    with ThreadPoolExecutor(3) as ex:
        parts = list(ex.map(build, ("render", "rgb_fwd", "rgb_bwd")))
    allk = {}
    for p in parts:
        allk.update(p)
    return allk


def _pick(kernels, base, targs):
    """The kernel `base` whose template argument list is exactly targs (e.g. 'Lb1ELb0E')."""
    hits = [k for k in kernels if k.startswith("_ZN2sc%d%s" % (len(base), base)) and ("I" + targs + "EEv") in k]
    assert len(hits) == 1, (base, targs, hits, sorted(kernels))
    return kernels[hits[0]]


# (kernel, template arguments of the S = 64 instance without the GEN flag)
FWD = [("rgb_composite_fwd_kernel", "Lb0E"), ("rgb_composite_fwd_kernel", "Lb1E"),
       ("rgb_composite_fwd_split_kernel", "Lb0E"), ("rgb_composite_fwd_split_kernel", "Lb1E")]
BWD = [("rgb_composite_bwd_kernel", "Lb0ELb0ELb0E"),        # _v3
       ("rgb_composite_bwd_kernel", "Lb1ELb0ELb0E"),        # _fused
       ("rgb_composite_bwd_kernel", "Lb1ELb1ELb0E"),        # _fused_stash
       ("rgb_composite_bwd_kernel", "Lb1ELb1ELb1E")]        # _fused_split
# The two fused reverse forms without register headroom at S = 64 (256 VGPRs and a few spilled) spill more in their chunked form:
# the per-ray carries of the chunk loop live across phase 2.  Measured with this compiler: _fused 84 B / 24 spills (S = 64: 28 / 6),
# _fused_split 64 B / 19 (S = 64: 20 / 4).  Bounded here so that a regression shows; the others are held to their S = 64 instance.
GEN_CEILING = {"Lb1ELb0ELb0E": (96, 28), "Lb1ELb1ELb1E": (72, 22)}


@pytest.mark.parametrize("base,targs", FWD + BWD)
def test_chunked_instance_uses_no_more_scratch_than_the_64_sample_instance(kernels, base, targs):
    s64 = _pick(kernels, base, targs + "Lb0E")
    gen = _pick(kernels, base, targs + "Lb1E")
    print(base, targs, "S=64 (scratch B, spills, VGPRs):", s64, "chunked:", gen)
    if base == "rgb_composite_bwd_kernel" and targs in GEN_CEILING:
        assert gen[0] <= GEN_CEILING[targs][0] and gen[1] <= GEN_CEILING[targs][1], (s64, gen)
    else:
        assert gen[0] <= s64[0] and gen[1] <= s64[1], (s64, gen)


def test_the_64_sample_instances_keep_their_resources(kernels):
    """The default path: the forward has no scratch, the reverse forms are where they were (0 / 0, 28 B / 6, 0 / 0, 20 B / 4)."""
    for base, targs in FWD:
        assert _pick(kernels, base, targs + "Lb0E")[:2] == (0, 0)
    want = [(0, 0), (28, 6), (0, 0), (20, 4)]
    for (base, targs), w in zip(BWD, want):
        assert _pick(kernels, base, targs + "Lb0E")[:2] <= w, (targs, _pick(kernels, base, targs + "Lb0E"))
    for k in ("ray_sample_kernel", "ray_sample_ns_kernel", "ray_sample_bwd_kernel", "ray_sample_bwd_ns_kernel"):
        hits = [v for n, v in kernels.items() if n.startswith("_ZN2sc%d%sE" % (len(k), k))]
        assert len(hits) == 1 and hits[0][:2] == (0, 0), (k, hits)


def test_sample_count_supported():
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.renderer import sample_count_supported
    for s in (32, 64, 96, 128, 160, 192, 224, 256):
        assert sample_count_supported(s) and ops.sample_count_supported(s)
    for s in (0, 16, 31, 48, 63, 65, 100, 288, 320, 512, -32, 64.0, "64", None):
        assert not sample_count_supported(s), s


def test_header_family_macro_matches_the_host_test():
    text = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    assert re.search(r"#define SC_N_SAMPLES_SUPPORTED\(n\) \(\(n\) >= 32 && \(n\) <= 256 && \(n\) % 32 == 0\)", text)
