"""CPU: the oracle's NL aggregation against the reference's OWN code, bit for bit.

Everything else here is compared with oracle/, a restatement written from reading the reference.
NL/ is the one part of the reference that builds without OpenCV: oracle/ref_nl.mk compiles adapted
copies of qx_mst_kruskals_image, qx_tree_filter, qx_basic and ctmf behind our driver into
oracle/_ref/ref_nl_driver (not in git), and oracle/ref_nl.py runs it.  These tests pin
    oracle.nl_median3   to ctmf as mst() calls it (NL/qx_mst_kruskals_image.cpp:174),
    oracle.nl_tree      to qx_mst_kruskals_image::mst's getters, node for node,
    oracle.nl_table and oracle.nl_aggregate to qx_tree_filter (as NLCCA::aggreCV drives it) and the
                        float quotient of NL() (stereoMatching.cpp:4892-4917),
with no tolerance, on image families from no ties to nothing but ties (tests/ref_nl_cases.py).

Two checks look at the reference build alone, so that agreement cannot be vacuous: transposing the
input (which swaps the two edge families) changes most of its output, and it fails in ctmf's
unsupported window, 363 <= rows * cols <= 543 px (oracle/ref_nl.py), and works on both sides of it.

With a reference checkout beside the repository and no binary the tests FAIL (build() should have
made it); with neither they skip, and test_oracle_matches_recorded_reference still compares the
oracle with tests/golden/ref_nl.npz, outputs of the binary recorded by tests/golden/make_ref_nl.py.
The same script records what tests/test_gpu_ref_nl.py expects (tests/golden/ref_nl_gpu.npz), for GPU
machines without the binary; the last two tests here keep that file complete and current."""
import os

import numpy as np
import pytest

import ref_nl_cases as K
from oracle import ref_nl as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_nl.npz")
TREE_KEYS = ("parent", "nchild", "child", "weight", "order", "rank")


def need_binary():
    if R.available():
        return
    if R.checkout_present():
        pytest.fail(f"a reference checkout is at {R.reference_dir()} but {R.BINARY} is not built: "
                    "build() (make -C oracle -f ref_nl.mk) must produce it")
    pytest.skip("no reference checkout and no oracle/_ref binary; tests/golden/ref_nl.npz stands in")


def assert_tree_equal(ot, rt, n):
    """oracle.nl_tree (child[n, 4]) against the reference's getters (children[n][3]), node for node."""
    np.testing.assert_array_equal(ot["order"], rt["order"])
    np.testing.assert_array_equal(ot["parent"], rt["parent"])
    np.testing.assert_array_equal(ot["weight"], rt["weight"])
    np.testing.assert_array_equal(ot["nchild"], rt["nchild"])
    assert int(rt["nchild"].max(initial=0)) <= 3
    valid = np.arange(3)[None, :] < rt["nchild"][:, None]
    np.testing.assert_array_equal(np.where(valid, ot["child"][:, :3], -1), rt["child"])
    # the reference's rank is the depth: one more than the parent's, 0 at the root
    depth = np.zeros(n, np.int32)
    for p in ot["order"][1:]:
        depth[p] = depth[ot["parent"][p]] + 1
    np.testing.assert_array_equal(depth, rt["rank"])


def oracle_nl(oracle, vol, bgr, sigma):
    H, W, P = vol.shape
    return oracle.nl_aggregate(vol, bgr, oracle.config(H, W, max(P - 1, 1), nl_sigma=sigma))


@pytest.mark.parametrize("H,W", K.SHAPES)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_median_and_tree_match_reference(oracle, family, H, W):
    need_binary()
    bgr = K.image(family, H, W)
    np.testing.assert_array_equal(oracle.nl_median3(bgr), R.median(bgr))
    assert_tree_equal(oracle.nl_tree(bgr), R.tree(bgr), H * W)


@pytest.mark.parametrize("sigma", K.SIGMAS)
@pytest.mark.parametrize("H,W", K.SHAPES)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_aggregate_matches_reference(oracle, family, H, W, sigma):
    """oracle.nl_aggregate == (float) filter(cost) / (float) filter(ones) of the reference build."""
    need_binary()
    bgr, vol = K.image(family, H, W), K.volume(H, W, 5)
    np.testing.assert_array_equal(K.bits(oracle_nl(oracle, vol, bgr, sigma)), K.bits(R.nl(vol, bgr, sigma)))


@pytest.mark.parametrize("family", ["make_pair", "random"])
def test_teddy_size_matches_reference(oracle, family):
    need_binary()
    H, W = 375, 450
    bgr, vol = K.image(family, H, W), K.volume(H, W, 4)
    np.testing.assert_array_equal(oracle.nl_median3(bgr), R.median(bgr))
    assert_tree_equal(oracle.nl_tree(bgr), R.tree(bgr), H * W)
    np.testing.assert_array_equal(K.bits(oracle_nl(oracle, vol, bgr, 0.1)), K.bits(R.nl(vol, bgr, 0.1)))


@pytest.mark.parametrize("sigma", K.SIGMAS)
def test_table_matches_reference(oracle, sigma):
    """qx_tree_filter's weight table is private; a 3 x 3 image reads it out one entry at a time.
    Columns (0, k, k) survive the clamped median, the vertical edges weigh 0 and (0,0)-(0,1) is the
    first edge of weight k, so pixel 1 is a child of the root with weight k; a single cost of 1 at
    pixel 1 then leaves the root exactly 0 + 1 * table[k].  The output is a float, so this pins
    (float) table[k]; the table's low bits are pinned by the bit-exact volumes above."""
    need_binary()
    table = oracle.nl_table(sigma)
    vol = np.zeros((3, 3, 1), np.float32)
    vol[0, 1, 0] = 1
    for k in range(256):
        bgr = np.zeros((3, 3, 3), np.uint8)
        bgr[:, 1:, :] = k
        t = oracle.nl_tree(bgr)           # pinned to the reference by test_median_and_tree_match_reference
        assert t["parent"][1] == 0 and t["weight"][1] == k, k
        if k in (0, 1, 128, 255):
            rt = R.tree(bgr)
            assert rt["parent"][1] == 0 and rt["weight"][1] == k, k
        got = R.filter(vol, bgr, sigma)[0, 0, 0]
        assert K.bits(got) == K.bits(np.float32(table[k])), (k, float(got), float(table[k]))
    assert table[0] == 1.0
    if sigma < 0.01:
        np.testing.assert_array_equal(table, oracle.nl_table(0.01))


@pytest.mark.parametrize("family", K.NON_FLAT)
def test_reference_depends_on_edge_order(family):
    """The reference alone: filtering the transposed input and transposing back swaps the two edge
    families (rows first, then columns), and must change at least a tenth of the elements -- else
    the inputs could not tell a misread tie order from the right one."""
    need_binary()
    H, W = 40, 61
    bgr, vol = K.image(family, H, W), K.volume(H, W, 5)
    a = R.filter(vol, bgr)
    b = R.filter(np.ascontiguousarray(vol.transpose(1, 0, 2)), np.ascontiguousarray(bgr.transpose(1, 0, 2)))
    frac = float((K.bits(a) != K.bits(b.transpose(1, 0, 2))).mean())
    print(f"{family}: transposition changes {100 * frac:.1f} % of the elements")
    assert frac >= 0.1


@pytest.mark.parametrize("H,W,works", [(19, 19, True), (11, 33, False), (3, 181, False), (17, 32, True)])
def test_reference_unsupported_window(H, W, works):
    """The reference alone: ctmf as mst() calls it aborts (assertions on) for 363..543 px -- measured
    at both ends of the window -- and works on the pixel counts next to it, 361 and 544."""
    need_binary()
    bgr = K.image("random", H, W)
    assert R.in_window(H, W) == (not works)
    if works:
        assert len(R.run_raw(bgr, "median", timeout=30)) == H * W * 3
        R.tree(bgr)
    else:
        with pytest.raises(R.RefNLError, match="failed"):
            R.run_raw(bgr, "median", timeout=30)
        with pytest.raises(R.RefNLError, match="363"):      # the wrapper refuses without starting it
            R.median(bgr)


def golden_cases():
    z = np.load(GOLDEN)
    return [{k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")} for i in range(int(z["n_cases"]))]


def test_oracle_matches_recorded_reference(oracle):
    """Runs everywhere: the oracle against outputs of the reference build recorded in
    tests/golden/ref_nl.npz (24 x 30 with P = 8, 3 x 90, 130 x 5)."""
    cases = golden_cases()
    assert len(cases) == 3
    for c in cases:
        bgr, vol, sigma = c["bgr"], c["vol"], float(c["sigma"])
        H, W, P = vol.shape
        assert K.sha256(bgr, vol, c["sigma"]) == str(c["sha256"])
        np.testing.assert_array_equal(oracle.nl_median3(bgr), c["median"])
        assert_tree_equal(oracle.nl_tree(bgr), c, H * W)
        want = c["filter"] / c["filter_ones"]            # NL(): float volume / float volume
        assert want.dtype == np.float32
        np.testing.assert_array_equal(K.bits(oracle_nl(oracle, vol, bgr, sigma)), K.bits(want))


def test_recorded_reference_is_current():
    """The recorded cases are what the binary gives today, on the inputs make_ref_nl.py generates."""
    need_binary()
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    try:
        import make_ref_nl
    finally:
        sys.path.pop(0)
    # ref_nl.npz, and ref_nl_gpu.npz: what tests/test_gpu_ref_nl.py expects where the binary is absent
    for now, path in ((make_ref_nl.record(), GOLDEN), (make_ref_nl.record_gpu(), make_ref_nl.OUT_GPU)):
        z = np.load(path)
        assert sorted(now) == sorted(z.files)
        for k in z.files:
            np.testing.assert_array_equal(np.asarray(now[k]), z[k], err_msg=k)


def test_recorded_gpu_cases_are_complete():
    """Runs everywhere: tests/golden/ref_nl_gpu.npz names every case of ref_nl_cases.gpu_cases(), on
    today's inputs, and each volume kept in full has the recorded digest."""
    z = dict(np.load(os.path.join(os.path.dirname(GOLDEN), "ref_nl_gpu.npz")))
    cases = K.gpu_cases()
    assert sorted(k[3:] for k in z if k.startswith("in_")) == sorted(cases)
    for key, (raw, bgr, sigma) in cases.items():
        assert K.input_digest(raw, bgr, sigma) == str(z[f"in_{key}"]), key
        if f"vol_{key}" in z:
            assert K.sha256(K.bits(z[f"vol_{key}"])) == str(z[f"sha_{key}"]), key
    for key in ("gfnl", "sigma_0.1", "sigma_0.5", "sigma_0.005", "batch_0", "batch_1", "batch_2"):
        assert f"vol_{key}" in z, key     # the GPU tests read these element by element
