"""CPU: the scenes of tests/scale_scenes.py, with the host mirrors alone.

What makes tests/test_gpu_scale.py meaningful is stated and checked here first: each scene reaches the regime it is
named for -- past box_partial_kernel's grid-stride threshold, on the radix sort's merge path over hundreds of blocks or on
onesweep, equal keys in every block of the sort, several refit launches of a height of their own, a rebuild that moves the
stacks from LDS to HBM, a leaf of 255.  If one fails, the scene is at fault, not the threshold.

rocPRIM's rocprim/device/device_radix_sort.hpp, which hipcub's DeviceRadixSort::SortPairs goes through, sorts n <= 1,024
in one block, 1,024 < n <= 1,048,576 by a block sort and merge passes, and anything larger by onesweep.

And the vectorised structure check of the GPU tests, scale_scenes.pairs_from_nodes, is held equal to the pair-by-pair loop
of tests/test_gpu_rebuild_leaf.py and to the walks of tests/rebuild_ref.py on every small scene.
"""
import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_models_ref as MR
import rebuild_ref as BR
import refit_ref as RR
import scale_scenes as SC
import srt_amd as S
from conftest import OBJECTS
from test_gpu_rebuild_leaf import pairs_loop

# (scene, max_leaf) of tests/test_gpu_scale.py's rebuilds -> stack.in_hbm of the creation tree and of the rebuilt one
IN_HBM = {("knot70k", 1): (0, 1), ("knot70k", 4): (0, 1), ("clusters", 1): (0, 0), ("clusters", 4): (0, 0)}


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def scenes(rubik):
    return {name: SC.make_scene(name, rubik) for name in ("knot70k", "clusters", "knot70k_and_rubik")}


@pytest.fixture(scope="module")
def built(scenes):
    """{(scene, max_leaf): (mirror-built scene, order)} of the one-record scenes."""
    return {(name, leaf): S.build_lbvh(*scenes[name], max_leaf=leaf) for name in ("knot70k", "clusters") for leaf in SC.LEAVES}


def test_triangle_counts_cross_the_thresholds(scenes):
    box_loop = SC.box_loop_threshold()
    assert box_loop == 65536 and SC.ONE_BLOCK == 1024 and SC.MERGE_LIMIT == 1_048_576
    for name in ("knot70k", "clusters"):
        n = len(scenes[name][0].tris)
        assert n == SC.N_KNOT == 69632 == 272 * 256 and box_loop < n <= SC.MERGE_LIMIT
    scene = scenes["knot70k"][0]
    assert 32 * len(scene.nodes) + 48 * len(scene.tris) >= 1 << 20  # csrc/scene_image.cpp: triangle slots, a top region
    assert SC.N_SOUP == 1_052_672 > SC.MERGE_LIMIT
    two = scenes["knot70k_and_rubik"][0]
    assert len(two.bvhs) == 2 and box_loop < len(two.tris) == SC.N_KNOT + 1188 <= SC.MERGE_LIMIT


def test_the_knot_box_needs_the_second_pass_of_the_loop(scenes):
    """Block b of box_partial_kernel folds triangles b * 256 + lane in its first pass and those past 65,536 in its
    second: the box of the first 65,536 alone is not the scene box, so a second pass lost would change the keys."""
    scene, verts = scenes["knot70k"]
    head = SC.box_loop_threshold()
    assert SC.box_needs_the_tail(scene, verts, head)
    assert not SC.box_needs_the_tail(scene, verts, len(scene.tris))
    # the scene is still the loader's: a valid tree over the same triangles, its leaves tiling the array
    leaf = scene.nodes[scene.nodes["count"] > 0]
    first = np.sort(leaf["first"].astype(np.int64))
    assert first[0] == 0 and len(np.unique(first)) == len(first) and int(leaf["count"].sum()) == len(scene.tris)
    assert sorted(scene.tri_input.tolist()) == list(range(len(scene.tris)))
    assert S.refit_scene(scene, scene.verts).nodes.tobytes() == scene.nodes.tobytes()


def test_the_soup_is_as_large_as_its_name():
    """(The tree is not needed: the model reports its triangles.)"""
    from srt_amd import render as R
    assert R.synthetic_triangles(SC.N_SOUP).shape == (SC.N_SOUP, 9) and SC.N_SOUP > SC.MERGE_LIMIT


def test_distinct_keys(scenes):
    for name, (scene, verts) in scenes.items():
        if len(scene.bvhs) == 1:
            distinct = len(np.unique(BR.keys(scene, verts)))
            if name == "clusters":
                assert distinct == SC.N_BASES == 17
            else:
                assert distinct > len(scene.tris) // 2


def test_clusters_put_every_key_into_every_block_of_the_sort(scenes, built):
    """Triangle t of the creation order is base t % 17, at the creation vertices and at the rebuild's: every run of 256
    (and of 17) consecutive triangles holds all 17 keys, 4,096 triangles share each, and the mirror's order is the stable
    one -- inside a key the creation indices ascend."""
    scene, verts = scenes["clusters"]
    for v in (scene.verts, verts):
        k = BR.keys(scene, v)
        assert (k == k[np.arange(len(k)) % SC.N_BASES]).all()
        assert len(np.unique(k[:SC.N_BASES])) == SC.N_BASES
        assert (np.bincount(np.unique(k, return_inverse=True)[1]) == 4096).all()
        p = BR.positions(scene, v)
        assert (p == p[np.arange(len(p)) % SC.N_BASES]).all()  # copies stay coincident
    k = BR.keys(scene, verts)
    for leaf in SC.LEAVES:
        order = built["clusters", leaf][1].astype(np.int64)
        assert (order == BR.order(k)).all()
        same = k[order][1:] == k[order][:-1]
        assert same.sum() == len(k) - SC.N_BASES and (np.diff(order)[same] > 0).all()


@pytest.mark.parametrize("max_leaf", SC.LEAVES)
def test_the_mirror_on_clusters_cut_down_is_the_restatement(max_leaf):
    """The same 17 bases, 64 copies each (1,088 triangles: past one block of the sort), where the numpy restatement of
    the rule is affordable: the order and the hierarchy of the mirror against it."""
    n = SC.N_BASES * 64
    scene = SC.heap_scene(S.model_from_triangles(SC.cluster_triangles(n)), SC.N_BASES)
    verts = RR.wave(scene.verts, 0.25, 0.3)
    k = BR.keys(scene, verts)
    assert len(np.unique(k)) == SC.N_BASES and n > SC.ONE_BLOCK
    built, order = S.build_lbvh(scene, verts, max_leaf=max_leaf)
    assert (order == BR.order(k)).all()
    if max_leaf == 1:
        assert BR.host_children(built.nodes) == BR.hierarchy(k[order])
    else:
        assert LR.host_tree(built.nodes) == LR.collapsed(k[order], max_leaf)


def test_the_knot_order_is_the_restatement(scenes, built):
    scene, verts = scenes["knot70k"]
    for leaf in SC.LEAVES:
        assert (built["knot70k", leaf][1] == BR.order(BR.keys(scene, verts))).all()


def test_heights_with_launches_of_their_own(scenes, built):
    """More than 256 pairs at three heights or more: the refit schedule has at least three per-height launches."""
    assert SC.heights_over(scenes["knot70k"][0]) >= 3          # the creation tree (midpoint splits)
    for key, (tree, _) in built.items():
        assert SC.heights_over(tree) >= 3, key
    for leaf in SC.LEAVES:
        tree, _ = S.build_lbvh_models(*scenes["knot70k_and_rubik"], max_leaf=leaf)
        assert SC.heights_over(tree) >= 3


def test_a_rebuild_moves_the_stacks_to_hbm(scenes, built):
    """The knot's creation tree is 20 deep (21 entries of 256 * 12 B: 64,512 B, LDS), the rebuilt ones 25 (max_leaf 1) and
    22 (max_leaf 4) deep: HBM.  The clusters stay in LDS either way."""
    for (name, leaf), want in IN_HBM.items():
        before = SC.in_hbm(LR.shape(scenes[name][0].nodes)[2])
        after = SC.in_hbm(LR.shape(built[name, leaf][0].nodes)[2])
        assert (before, after) == want, (name, leaf)
    assert any(a != b for a, b in IN_HBM.values())
    assert LR.shape(scenes["knot70k"][0].nodes)[2] == 20 and LR.shape(built["knot70k", 4][0].nodes)[2] == 22


def test_record_0_fills_whole_blocks_and_rubik_lies_outside(scenes):
    scene, verts = scenes["knot70k_and_rubik"]
    own = MR.owners(scene)
    assert (own[:SC.N_KNOT] == 0).all() and (own[SC.N_KNOT:] == 1).all() and SC.N_KNOT % 256 == 0
    assert len(scene.tris) % 256 != 0  # Rubik's last block is a partial one
    for v in (scene.verts, verts):
        p = BR.positions(scene, v)
        assert p[own == 1][..., 0].min() > p[own == 0][..., 0].max() + 1.0


def test_the_shuffle_interleaves_the_two_records_in_every_block(scenes, rubik):
    """"knot70k_and_rubik_shuffled": the same triangles under the same records, Rubik's spread over the whole array -- no
    block of 256 has one owner for sure where Rubik's 1,188 triangles fall, and they fall into at least 100 of the 277
    blocks -- and the mirror builds the same two trees as from the creation order, the order mapped through the shuffle."""
    scene, verts = scenes["knot70k_and_rubik"]
    got, verts_s = SC.make_scene("knot70k_and_rubik_shuffled", rubik)
    assert verts_s.tobytes() == verts.tobytes()
    own, own_s = MR.owners(scene), MR.owners(got)
    assert np.bincount(own_s).tolist() == np.bincount(own).tolist() == [SC.N_KNOT, 1188]
    mixed = sum(1 for i in range(0, len(own_s), 256) if len(set(own_s[i:i + 256].tolist())) == 2)
    assert mixed >= 100
    assert (got.tri_input[own_s == 1] >= SC.N_KNOT).all() and (got.tri_input[own_s == 0] < SC.N_KNOT).all()
    a, oa = S.build_lbvh_models(scene, verts, max_leaf=4)
    b, ob = S.build_lbvh_models(got, verts, max_leaf=4)
    # equal keys (the knot has some) keep the array's order, which the shuffle changed: the trees' shapes and boxes agree,
    # the triangles agree as sets per record
    assert a.nodes["count"].tobytes() == b.nodes["count"].tobytes() and len(a.nodes) == len(b.nodes)
    assert a.bvhs.tobytes() == b.bvhs.tobytes()
    for f in ("min", "max"):
        assert (a.nodes[f][0] == b.nodes[f][0]).all()
    assert sorted(scene.tri_input[oa].tolist()) == sorted(got.tri_input[ob].tolist())


def test_a_leaf_of_255():
    scene, verts = SC.leaf255_scene()
    tree, order = S.build_lbvh(scene, verts, max_leaf=255)
    assert len(scene.tris) == 511 and len(np.unique(BR.keys(scene, verts))) == 1
    root, pairs = LR.host_tree(tree.nodes)
    assert pairs[0][1] == ("leaf", 256, 255) and LR.shape(tree.nodes)[1] == 255
    assert (root, pairs) == LR.collapsed(BR.keys(scene, verts)[order], 255)


# -- the vectorised structure check ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", (1, 2, 4))
@pytest.mark.parametrize("name", BR.SCENES)
def test_pairs_from_nodes_is_the_loop_and_the_walk(rubik, name, max_leaf):
    scene, verts = BR.make_scene(name, rubik)
    tree, _ = S.build_lbvh(scene, verts, max_leaf=max_leaf)
    pairs = SC.pairs_from_nodes(tree.nodes)
    m = (len(tree.nodes) - 1) // 2
    assert pairs.shape == (4 * m, 4) and pairs.dtype == np.uint32 and (pairs == pairs_loop(tree.nodes)).all()
    root = SC.root_from_nodes(tree.nodes)
    BR.assert_same_tree(BR.walk_layout(pairs, root), BR.walk_nodes(tree.nodes))
    if max_leaf == 1:  # Karras' numbering is the same one: pair i holds node i's children
        kids = BR.host_children(tree.nodes)
        for i, sides in kids.items():
            for slot, (index, leaf) in enumerate(sides):
                assert (int(pairs[4 * i + 2 * slot, 3]), int(pairs[4 * i + 2 * slot + 1, 3])) == (index, 1 if leaf else 0)
    if m:
        SC.assert_is_a_tree(pairs, m, len(tree.tris))


def test_pairs_from_nodes_at_scale(built):
    for key, (tree, _) in built.items():
        pairs = SC.pairs_from_nodes(tree.nodes)
        SC.assert_is_a_tree(pairs, (len(tree.nodes) - 1) // 2, len(tree.tris))
        if key == ("knot70k", 4):
            assert (pairs == pairs_loop(tree.nodes)).all()
            BR.assert_same_tree(BR.walk_layout(pairs, SC.root_from_nodes(tree.nodes)), BR.walk_nodes(tree.nodes))


def test_height_counts_is_the_walk(rubik, built):
    """The vectorised pairs per height (used alone at 1 M triangles) against refit_ref.pair_height_counts, and the
    schedule from them against test_gpu_rebuild.expected_schedule."""
    from test_gpu_rebuild import expected_schedule

    trees = [tree for tree, _ in built.values()]
    trees += [S.build_lbvh(*BR.make_scene(name, rubik), max_leaf=leaf)[0] for name in BR.SCENES for leaf in (1, 4)]
    for tree in trees:
        counts = SC.height_counts(tree.nodes)
        if len(tree.nodes) > 1:
            assert counts.tolist() == RR.pair_height_counts(tree).tolist()
        assert SC.schedule_of(counts) == expected_schedule(tree)


def test_is_a_tree_notices_a_lost_and_a_doubled_pair(built):
    tree, _ = built["knot70k", 4]
    m = (len(tree.nodes) - 1) // 2
    pairs = SC.pairs_from_nodes(tree.nodes)
    inner = np.flatnonzero(pairs[1::2, 3] == 0)
    bad = pairs.copy()
    bad[2 * inner[5], 3] = bad[2 * inner[6], 3]
    with pytest.raises(AssertionError):
        SC.assert_is_a_tree(bad, m, len(tree.tris))
    leaf = np.flatnonzero(pairs[1::2, 3] > 0)
    bad = pairs.copy()
    bad[2 * leaf[7], 3] += 1
    with pytest.raises(AssertionError):
        SC.assert_is_a_tree(bad, m, len(tree.tris))
