"""The launch partitions of the two fused reverse kernels (csrc/sdf_bwdw.hip, the FUSED forms of csrc/rgb_bwd.hip) on the host: no GPU.
tests/reverse_routing_cases.py restates them in plain Python; checked here: every case of tests/test_gpu_reverse_image_routing.py runs
the per-image routing branch it is named for (idle workgroups, the share of mixed iterations, a flush per iteration, dense or atomic
form), and the restated workgroup counts and partial strides are the library's own -- so the case tables stop passing, instead of
quietly testing something else, when BW_CHAIN or one of the 256 caps is retuned."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reverse_routing_cases as C  # noqa: E402


@pytest.mark.parametrize("B,N", list(C.SDF_CASES))
def test_sdf_case_table_is_what_the_partition_gives(B, N):
    p = C.sdf_partition(B, N)
    print((B, N), p)
    assert p["covered"], "every tile belongs to exactly one workgroup"
    assert {k: p[k] for k in C.SDF_CASES[(B, N)]} == C.SDF_CASES[(B, N)]
    assert p["stride"] == C.SDF_PACK_FLOATS + (320 * B if p["dense"] else 0) and p["dense"] == (B <= 256)


def test_sdf_cases_hit_the_branches_they_are_named_for():
    P = {k: C.sdf_partition(*k) for k in C.SDF_CASES}
    # (5, 16): 5 tiles on 2 workgroups -- one iteration across 4 images, then a lone tile (three empty chain slots) that is one image
    p = P[(5, 16)]
    assert (p["ntiles"], p["blocks"], p["per_wg"], p["iters"], p["mixed"], p["span"], p["flushes"]) == (5, 2, 4, 2, 1, 4, 1)
    # (7, 48): 3 tiles per image -- no full iteration fits an image (mixed across 2), the lone last tile does
    p = P[(7, 48)]
    assert p["mixed"] == p["iters"] - 1 and p["span"] == 2 and p["flushes"] == 1
    # (64, 32), (256, 16), (300, 32): every iteration mixed, across 2 / 4 / 2 images, no accumulator ever carries a sum
    for k, span in (((64, 32), 2), ((256, 16), 4), ((300, 32), 2)):
        assert P[k]["mixed"] == P[k]["iters"] > 1 and P[k]["span"] == span and P[k]["flushes"] == 0, k
    # (130, 64), (260, 64): 4 tiles per image -- never mixed, a flush for every iteration
    for k in ((130, 64), (260, 64)):
        assert P[k]["mixed"] == 0 and P[k]["flushes"] == P[k]["iters"] == k[0], k
    # (256, 16) is the largest dense form, (257, 16) the smallest atomic one (one lone tile behind 64 mixed iterations)
    assert P[(256, 16)]["dense"] and P[(256, 16)]["stride"] == C.SDF_PACK_FLOATS + 81920
    assert not P[(257, 16)]["dense"] and P[(257, 16)]["stride"] == C.SDF_PACK_FLOATS
    assert (P[(257, 16)]["mixed"], P[(257, 16)]["iters"], P[(257, 16)]["flushes"]) == (64, 65, 1)
    assert not P[(300, 32)]["dense"] and not P[(260, 64)]["dense"]
    # (5, 3296): 1030 tiles -- 256 workgroups of 8 tiles, 127 of them idle, dense; accumulators that live across iterations (258 iterations,
    # 130 flushes), two mixed iterations and one change of image between two pure iterations of a workgroup
    p = P[(5, 3296)]
    assert (p["ntiles"], p["blocks"], p["per_wg"], p["idle"], p["dense"], p["mixed"]) == (1030, 256, 8, 127, True, 2)
    assert p["flushes"] == (256 - 127) + 1 and p["iters"] == 2 * (256 - 127)
    # (260, 64): 1040 tiles -- idle workgroups and the atomic form together
    p = P[(260, 64)]
    assert (p["ntiles"], p["blocks"], p["per_wg"], p["idle"], p["dense"]) == (1040, 256, 8, 126, False)
    # what the shapes the suite ran before never had: an idle workgroup, and more than 256 images
    assert sum(p["idle"] > 0 for p in P.values()) == 2 and sum(not p["dense"] for p in P.values()) == 3
    assert set(C.SDF_LEAK_CASES) <= set(P) and set(C.SDF_BATCH_CASES) <= set(P) and C.SDF_FEAT_ABSENT in P
    assert any(P[k]["dense"] for k in C.SDF_LEAK_CASES) and any(not P[k]["dense"] for k in C.SDF_LEAK_CASES)
    assert any(P[k]["idle"] for k in C.SDF_LEAK_CASES) and any(P[k]["idle"] for k in C.SDF_BATCH_CASES)


def test_shapes_the_suite_ran_before_leave_the_gap():
    """The (B, N) of the fused SDF reverse in the suite before this file: no idle workgroup, at most two mixed iterations, all dense."""
    for B, N in [(1, 16), (1, 48), (2, 96), (2, 512), (3, 1040), (2, 16384), (2, 40960), (4, 512 * 64), (16, 512 * 64), (32, 512 * 64),
                 (4, 1024), (16, 1024), (32, 1024)]:
        p = C.sdf_partition(B, N)
        assert p["idle"] == 0 and p["mixed"] <= 2 and p["dense"] and p["covered"], (B, N, p)
    for n_images, rpi in [(3, 40), (3, 37), (2, 512)]:
        p = C.rgb_partition(n_images, rpi)
        assert p["mixed"] <= 2 and p["covered"], (n_images, rpi, p)


@pytest.mark.parametrize("n_images,rpi,S", list(C.RGB_CASES))
def test_rgb_case_table_is_what_the_partition_gives(n_images, rpi, S):
    p = C.rgb_partition(n_images, rpi)
    print((n_images, rpi, S), p)
    assert p["covered"], "every ray belongs to exactly one (iteration, block, wave)"
    assert {k: p[k] for k in C.RGB_CASES[(n_images, rpi, S)]} == C.RGB_CASES[(n_images, rpi, S)]
    assert n_images <= C.DENSE_MAX_IMAGES and rpi < 4          # the fused form; fewer than 4 rays per image
    # fewer than 4 rays per image: every full iteration is mixed (only a ragged last one can lie in one image)
    assert p["mixed"] >= p["iters"] - 1 and p["mixed"] >= 1
    assert p["span"] == {1: 4, 2: 2, 3: 2}[rpi]


def test_rgb_cases_reach_the_largest_fused_batch():
    assert max(k[0] for k in C.RGB_CASES) == C.DENSE_MAX_IMAGES
    assert {k[2] for k in C.RGB_CASES if k[0] == C.DENSE_MAX_IMAGES} == {32, 64}
    assert set(C.RGB_LEAK_CASES) <= set(C.RGB_CASES)


def test_restated_partitions_are_the_librarys():
    """Workgroup counts and partial strides against the C ABI's own queries (host functions: no device is asked)."""
    from shapeclipper_amd import _lib, packing
    lib = _lib.load()
    assert C.SDF_PACK_FLOATS == packing.SDF_PACK_FLOATS and C.RGB_V3_OFFSET == packing.RGB_OFF["V3"] and C.TILE == packing.TILE
    sizes = sorted({B * N for B, N in C.SDF_CASES} | {1, 15, 16, 17, 64, 65, 16 * 1023, 16 * 1024, 16 * 1024 + 1, 16 * 1025, 1 << 20})
    for n in sizes:
        assert lib.sc_sdf_backward_fused_parts(n) == C.sdf_parts(n), n
    for n_rays in sorted({k[0] * k[1] for k in C.RGB_CASES} | {1, 3, 4, 5, 1023, 1024, 1025, 4096}):
        assert lib.sc_rgb_composite_backward_fused_parts(n_rays) == C.rgb_parts(n_rays), n_rays
    for B in sorted({k[0] for k in C.SDF_CASES} | {k[0] for k in C.RGB_CASES} | {1, 255, 256, 257, 1000}):
        assert lib.sc_sdf_backward_fused_partial_floats(B) == C.sdf_partial_floats(B), B
        assert lib.sc_rgb_composite_backward_fused_partial_floats(B) == C.rgb_partial_floats(B), B
    for B, N in C.SDF_CASES:
        p = C.sdf_partition(B, N)
        assert lib.sc_sdf_backward_fused_parts(B * N) == p["blocks"] and lib.sc_sdf_backward_fused_partial_floats(B) == p["stride"]
