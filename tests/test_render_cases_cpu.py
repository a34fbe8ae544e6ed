"""CPU (no GPU): the scenes of tests/render_cases.py reach the edges of the tiled rasteriser they are named after, by the host
census of the binning decisions, and the census agrees with the restatement (tests/render_rgb_np.py) about what is drawn.  These
are the preconditions of tests/test_gpu_render_edges.py; a scene that misses one is changed, not the condition.  Also the
renderer's shape rule, which needs no device."""
import numpy as np
import pytest

from tests import render_cases as C
from tests import render_rgb_np as RR

G_CHECKED = C.G_ALONE + C.G_OFF_SCREEN


def fragments(name, pose=0):
    return list(RR.fragments(*C.pose_args(C.scene(name), pose)))


def test_constants_are_those_of_the_sources():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyrapose_amd", "csrc")
    text = open(os.path.join(csrc, "render.hip")).read() + open(os.path.join(csrc, "pose_common.h")).read()
    for name in ("RT", "RASTER_THREADS", "RASTER_SMALL_PX", "BIN_MAX_TILES", "SCAN_THREADS"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(C, name), name


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_census_draws_what_the_restatement_draws(name):
    s = C.scene(name)
    for pose in (G_CHECKED if name == "G_scan_carry" else range(len(s["R"]))):
        cen = C.scene_census(name, pose)
        assert cen["drawn"] == [f[0] for f in fragments(name, pose)], (name, pose)
        assert cen["list_len"].sum() == len(cen["entries"]) and set(cen["big"]) <= set(cen["drawn"])
        assert all((cen["tiles"][tri] > C.BIN_MAX_TILES) == (tri in cen["big"]) for tri in cen["drawn"])
        assert all(1 <= e[3] <= C.RT * C.RT for e in cen["entries"])
    assert s["w"] <= 160 and s["h"] <= 160 and len(s["faces"]) <= 1000


def test_a_a_tile_list_takes_a_second_chunk():
    cen = C.scene_census("A_long_list")
    assert len(C.scene("A_long_list")["faces"]) == 338 and cen["drawn"] == list(range(338)) and not cen["big"]
    assert cen["list_len"][0, 0] == 338 > C.RASTER_THREADS and cen["list_len"].sum() == 338       # all inside one tile
    assert not any(e[4] for e in cen["entries"])                                                   # and on the small path
    depth, ids = C.restated("A_long_list")
    assert len(np.unique(ids[ids >= 0])) > 300 and (ids >= C.RASTER_THREADS).any() and len(np.unique(depth)) > 500
    # the variant: lists of more than one chunk in several tiles, triangles across the seam of two tiles either way and on the corner
    cen = C.scene_census("A_long_list_on_seams")
    assert (cen["list_len"] > C.RASTER_THREADS).sum() >= 2 and not cen["big"] and not any(e[4] for e in cen["entries"])
    where = {}
    for tri, ty, tx, _, _ in cen["entries"]:
        where.setdefault(tri, set()).add((ty, tx))
    spans = set(frozenset(v) for v in where.values())
    assert frozenset([(0, 0), (0, 1)]) in spans and frozenset([(0, 0), (1, 0)]) in spans and frozenset([(0, 1), (1, 1)]) in spans
    assert frozenset([(0, 0), (0, 1), (1, 0), (1, 1)]) in spans
    assert len(cen["drawn"]) < len(C.scene("A_long_list_on_seams")["faces"])                       # some lie below the image


def test_b_the_big_list_takes_a_second_chunk():
    cen = C.scene_census("B_long_big_list")
    assert len(cen["big"]) > C.RASTER_THREADS and len(cen["big"]) >= 300
    assert all(cen["tiles"][tri] == 9 for tri in cen["big"])
    depth, ids = C.restated("B_long_big_list")
    winners = np.unique(ids[ids >= 0])
    assert (ids >= 0).all() and (winners < C.RASTER_THREADS).sum() >= 30 and (winners >= C.RASTER_THREADS).sum() >= 30
    # fragments of equal float32 depth meet where cells touch: the key's low word decides there
    at_minimum = np.zeros((96, 96), np.int64)
    for _, rs, cs, keep, z32 in fragments("B_long_big_list"):
        at_minimum[rs, cs] += keep & (z32 == depth[rs, cs])
    assert at_minimum.min() == 1 and (at_minimum > 1).sum() >= 10, (at_minimum > 1).sum()


def test_c_boxes_on_both_sides_of_the_small_threshold():
    cen = C.scene_census("C_small_queued_threshold")
    areas = {}
    for tri, ty, tx, area, queued in cen["entries"]:
        areas.setdefault(tri, []).append((ty, tx, area, queued))
        assert queued == (area > C.RASTER_SMALL_PX)
    for tri, want in C.C_BOXES.items():
        assert areas[tri] == [(0, 0, want, want > 64)], tri
    assert sorted(a[2] for v in areas.values() for a in v).count(64) >= 3 and 65 in [a[2] for v in areas.values() for a in v]
    assert areas[C.C_STRADDLER] == [(0, 0, 32, False), (0, 1, 72, True)]                           # one triangle, both paths
    assert areas[5] == [(1, 1, 64, False)] and areas[6] == [(1, 1, 65, True)] and not cen["big"]
    ids = C.restated("C_small_queued_threshold")[1]
    assert set(np.unique(ids)) == set(range(-1, 7))                                                # every one shows somewhere


def test_d_tile_counts_on_both_sides_of_the_big_threshold():
    cen = C.scene_census("D_list_big_threshold")
    assert cen["tiles"] == C.D_TILES and cen["big"] == [3, 4, 5]
    assert sorted(set(cen["tiles"].values())) == [4, 5, 6]
    per_tri = {}
    for tri, ty, tx, _, _ in cen["entries"]:
        per_tri.setdefault(tri, []).append((ty, tx))
    assert per_tri == {0: [(0, 0), (0, 1), (1, 0), (1, 1)], 1: [(2, 0), (2, 1), (2, 2), (2, 3)], 2: [(0, 4), (1, 4), (2, 4), (3, 4)]}
    assert set(np.unique(C.restated("D_list_big_threshold")[1])) == set(range(-1, 6))


@pytest.mark.parametrize("name", ["E_fan", "E_fan_reversed_winding", "E_fan_reversed_order"])
def test_e_the_fan_covers_each_pixel_once(name):
    s = C.scene(name)
    x, y, _ = RR.project(s["pts"], s["K"], s["R"][0], s["t"][0])
    assert np.array_equal(x, np.array([32.5] + [p[0] for p in C.E_RIM], np.float32))              # exactly on pixel centres
    assert np.array_equal(y, np.array([32.5] + [p[1] for p in C.E_RIM], np.float32))
    count = np.zeros((64, 64), np.int64)
    for _, rs, cs, keep, z32 in fragments(name):
        count[rs, cs] += keep
        assert np.all(z32[keep] == np.float32(128.0))
    want = np.zeros((64, 64), np.int64)
    want[:63, :63] = 1                                  # the right-hand and the bottom line of centres are no top or left edges
    assert count.sum() == 3969 and np.array_equal(count, want)
    depth, ids = C.restated(name)
    assert len(np.unique(ids[ids >= 0])) == 8 and np.array_equal(ids >= 0, want == 1)
    # every spoke owns pixel centres: a centre exactly on an edge is given to one side by the top-left rule alone
    on_edge = 0
    for tri, f in enumerate(s["faces"]):
        V, sgn, edges, _ = RR._setup(x, y, np.full(9, 1.0 / 128.0), f)
        rr, cc = np.nonzero(ids == tri)
        on_edge += int((np.array(RR._weights(sgn, edges, rr, cc)) == 0.0).any(0).sum())
    assert on_edge > 150, on_edge


def test_e_orderings_show_the_same_surface():
    a, b, c = (C.restated(n) for n in ("E_fan", "E_fan_reversed_winding", "E_fan_reversed_order"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    assert np.array_equal(a[1], b[1])                                   # the winding does not move a pixel to another triangle
    assert np.array_equal(np.where(a[1] >= 0, 7 - a[1], -1), c[1])      # nor does the order of the faces


@pytest.mark.parametrize("w,h", C.F_SHAPES)
def test_f_image_shapes_are_partial_tiles(w, h):
    depth, ids = C.restated("F_%dx%d" % (w, h))
    assert depth.shape == (h, w) and (ids >= 0).sum() >= min(w * h, 600) * 0.6
    assert (ids[:, -1] >= 0).any()                                                                 # drawn up to the last column
    assert (ids[-1] >= 0).any()                                                                    # and to the last row


def test_f_shapes_cover_both_store_paths_and_idle_threads():
    ws, hs = [s[0] for s in C.F_SHAPES], [s[1] for s in C.F_SHAPES]
    assert any(w % 4 == 0 and w % 32 for w in ws) and any(w % 4 for w in ws) and 32 in ws and 32 in hs
    assert any(w % 32 and w % 32 <= 28 for w in ws)                     # threads of the right-hand tile that start at c >= width
    assert any(h % 32 and h % 32 < 32 for h in hs) and 1 in ws and 1 in hs


def test_g_the_scan_takes_a_second_chunk():
    s = C.scene("G_scan_carry")
    assert len(s["R"]) >= 171 and C.n_bins(s) > C.SCAN_THREADS and len(np.unique(s["t"], axis=0)) == len(s["R"])
    seam = C.scene_census("G_scan_carry", C.G_SEAM)
    assert C.G_SEAM * seam["n_tiles"] + 4 == C.SCAN_THREADS              # bin 1024 is this pose's tile (1, 1), bin 1023 its tile (1, 0)
    assert seam["list_len"][1, 0] > 5 and seam["list_len"][1, 1] > 5
    assert not set(C.G_ALONE) & set(C.G_OFF_SCREEN)
    for pose in G_CHECKED:
        cen = C.scene_census("G_scan_carry", pose)
        if pose in C.G_OFF_SCREEN:
            assert not cen["drawn"] and not cen["list_len"].any()
        else:
            assert len(cen["drawn"]) > 10 and (C.restated("G_scan_carry", pose)[1] >= 0).sum() > 100


def test_h_far_vertices_are_clamped_and_overflow_is_skipped():
    s = C.scene("H_far_coordinates")
    cen = C.scene_census("H_far_coordinates")
    x, y, iz = RR.project(s["pts"], s["K"], s["R"][0], s["t"][0])
    far = [np.abs(np.concatenate([x[s["faces"][tri]], y[s["faces"][tri]]])).max() for tri in C.H_FAR]
    assert all(0.5 * want < got < 2.0 * want for got, want in zip(far, (1e6, 1e9, 1e12))), far
    assert cen["drawn"] == [0] + list(C.H_FAR)
    assert [int((iz[s["faces"][tri]] == 0).sum()) for tri in C.H_SKIPPED] == [1, 1, 1]
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(s["K"][0, 0] * s["pts"][14, 0] / s["pts"][14, 2] + s["K"][0, 2]))   # beyond float32, not beyond float64
    assert s["pts"][17, 2] < 0 and s["pts"][20, 2] == 0
    ids = C.restated("H_far_coordinates")[1]
    assert all((ids == tri).sum() > 20 for tri in (0,) + C.H_FAR)


def test_i_bad_faces_are_skipped_among_good_ones():
    s = C.scene("I_bad_faces")
    cen = C.scene_census("I_bad_faces")
    n = len(s["pts"])
    assert cen["drawn"] == list(C.I_GOOD)
    assert (s["faces"] == -1).any() and (s["faces"] == n).any() and (s["faces"] > n).any()
    assert len(set(s["faces"][5])) == 2 and len(set(s["faces"][4])) == 3
    ids = C.restated("I_bad_faces")[1]
    assert set(np.unique(ids)) == set((-1,) + C.I_GOOD)
    from pyrapose_amd.utils.renderer import _mesh
    with pytest.raises(ValueError):                                     # why the GPU test goes through ops directly
        _mesh(s)


@pytest.mark.parametrize("name", ["J_coplanar_overlap", "J_coplanar_overlap_swapped"])
def test_j_the_smaller_index_wins_a_tie(name):
    frags = fragments(name)
    assert [f[0] for f in frags] == [0, 1]
    full = []
    for _, rs, cs, keep, z32 in frags:
        m = np.zeros((48, 64), bool)
        m[rs, cs] = keep
        full.append(m)
        assert np.all(z32[keep] == np.float32(512.0))
    overlap = full[0] & full[1]
    depth, ids = C.restated(name)
    assert overlap.sum() > 300 and (full[0] & ~full[1]).sum() > 100 and (full[1] & ~full[0]).sum() > 100
    assert np.all(ids[overlap] == 0) and np.all(ids[full[1] & ~full[0]] == 1) and np.all(depth[full[0] | full[1]] == np.float32(512.0))
    a, b = C.scene("J_coplanar_overlap"), C.scene("J_coplanar_overlap_swapped")
    assert np.array_equal(a["pts"][:3], b["pts"][3:]) and np.array_equal(a["pts"][3:], b["pts"][:3])


def test_j_fragments_exactly_on_the_clip_planes_are_kept():
    depth, ids = C.restated("J_clip_equality")
    near, far = np.zeros((48, 64), bool), np.zeros((48, 64), bool)
    near[5:41, 3:29] = True                                             # pixel centres inside 3.25 .. 28.75 x 5.25 .. 40.75
    far[5:41, 34:61] = True
    assert np.array_equal(depth == np.float32(C.J_NEAR), near) and np.array_equal(depth == np.float32(C.J_FAR), far)
    assert np.array_equal(ids >= 0, near | far)
    s = C.scene("J_clip_equality")
    assert s["near"] == C.J_NEAR and s["far"] == C.J_FAR and set(np.unique(s["pts"][:, 2])) == {C.J_NEAR, C.J_FAR}


def test_the_bin_count_is_bounded():
    """n_pose * tiles must fit an int: the scan takes it as one and the bin kernel indexes with it"""
    from pyrapose_amd import _lib
    lib = _lib.lib
    tiles = lambda w, h: ((w + 31) // 32) * ((h + 31) // 32)
    assert 65535 * tiles(16384, 16384) >= 2 ** 31 > 65535 * tiles(16384, 1024)
    for ws in (lib.pp_render_workspace_bytes, lib.pp_render_rgbd_workspace_bytes,
               lambda *a: lib.pp_render_rgbd_tex_workspace_bytes(*a, 2, 2)):
        assert ws(65535, 3, 1, 16384, 16384) == 0 and ws(1, 3, 1, 16384, 16384) > 0
        # the bound itself, at the same number of poses: 65535 x 32768 tiles = 2^31 - 32768; one more row of tiles passes 2^31
        assert 65535 * tiles(8192, 4096) == 2 ** 31 - 32768 and ws(65535, 3, 1, 8192, 4096) > 0 and ws(65535, 3, 1, 8192, 4097) == 0
        assert 32768 * tiles(8192, 8192) == 2 ** 31 and ws(32768, 3, 1, 8192, 8192) == 0 and ws(32767, 3, 1, 8192, 8192) > 0
