"""HyperDepth forest evaluation on the GPU (ctd_hyperdepth_eval_f32): bit for bit against the reference's output
(tests/golden/hyperdepth.npz) through the drop-in eval_forest and the packed tables, and against the numpy
restatement (tests/hyperdepth_ref.py) on seeded random forests larger than the fixture."""
import numpy as np
import pytest
import torch

from connecting_the_dots_amd import hyperdepth as hd
from tests import hyperdepth_ref as R
from tests.test_hyperdepth_host import golden_cases, normalised_rows, same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(golden_cases()), ids=lambda c: c["name"])
def test_drop_in_matches_reference_fixture(case, tmp_path):
    H = case["ims"].shape[1]
    prefix = str(tmp_path / "forest")
    for r in range(H):
        hd.save_forest(case["forests"][case["rows"][r]], "%s%d.bin" % (prefix, r))
    disps = np.zeros(case["ims"].shape, np.float32)
    out = hd.eval_forest(case["ims"], disps, n_disp_bins=case["bins"], depth_switch=0, n_threads=18,
                         forest_prefix=prefix, row_from=case["row_from"], row_to=case["row_to"])
    r0, r1 = normalised_rows(case)
    assert out.dtype == np.float32 and out.shape == case["ims"].shape + (3,)
    assert same_bits(out[:, r0:r1], case["expected"])
    assert np.isnan(out[:, :r0]).all() and np.isnan(out[:, r1:]).all()
    # the packed tables, built from the in-memory forests
    f = hd.HyperDepthForests([case["forests"][i] for i in case["rows"]], 0, "cuda")
    o2 = f.eval(torch.from_numpy(case["ims"]).cuda(), case["bins"], case["row_from"], case["row_to"])
    assert same_bits(o2.cpu().numpy(), out)


def _random_rows(seed, n_forests, H, **kw):
    rs = np.random.RandomState(seed)
    fs = [R.random_forest(rs, **kw) for _ in range(n_forests)]
    return rs, [fs[r % n_forests] for r in range(H)]


def _check(forests, ims, bins, row_from, row_to):
    tab = hd.HyperDepthForests(forests, 0, "cuda")
    got = tab.eval(torch.from_numpy(ims).cuda(), bins, row_from, row_to).cpu().numpy()
    want = R.eval_rows(forests, 0, ims, bins, row_from, row_to)
    assert same_bits(got, want)
    return got


def test_full_frames_against_restatement():
    """480 x 640, N = 2, C = 6400, 6 trees of depth 8, mean lists of 32, offsets beyond the patch, NaN thresholds"""
    H, W, bins = 480, 640, 10
    rs, forests = _random_rows(11, 6, H, n_trees=6, depth=8, C=W * bins, mean_len=32, off_lo=-24, off_hi=56)
    for f in forests[:6]:
        f.trees[0][0].threshold = np.float32(np.nan)            # tree 0 of every forest: its root always goes right
    ims = rs.randint(0, 256, (2, H, W)).astype(np.uint8)
    _check(forests, ims, bins, 0, H)


def test_long_lists_against_restatement():
    """>= 2000 entries per leaf (sum of 6 lists ~15000 per pixel), C = 6400, N = 3, a band of rows of a 480 x 640
    frame"""
    H, W, bins = 480, 640, 10
    rs, forests = _random_rows(12, 2, H, n_trees=6, depth=3, C=W * bins, mean_len=2600)
    assert min(len(nd.classes) for f in forests[:2] for t in f.trees for nd in t if isinstance(nd, hd.Leaf)) >= 1300
    assert np.mean([len(nd.classes) for f in forests[:2] for t in f.trees for nd in t if isinstance(nd, hd.Leaf)]) \
        >= 2000
    ims = rs.randint(0, 256, (3, H, W)).astype(np.uint8)
    _check(forests, ims, bins, 236, 244)


def test_sixteen_trees_at_the_lds_limit():
    """16 trees, C = 12288 (4 C + 1024 T = 64 KiB), unequal depths, single-class leaves, odd width"""
    H, W, bins = 40, 1229, 10
    rs, forests = _random_rows(13, 3, H, n_trees=16, depth=6, C=12288, mean_len=40, min_depth=2, one_class=0.3)
    ims = rs.randint(0, 256, (2, H, W)).astype(np.uint8)
    _check(forests, ims, bins, 0, H)


def test_ties_and_zero_rules_against_restatement():
    """counts 1..20 over few classes (many ties), some all-zero leaves, bins 4"""
    H, W, bins = 64, 200, 4
    C = W * bins
    rs, forests = _random_rows(14, 4, H, n_trees=5, depth=5, C=C, mean_len=3, one_class=0.3)
    for f in forests[:4]:
        for t in f.trees:
            for nd in t:
                if isinstance(nd, hd.Leaf):
                    if rs.rand() < 0.2:
                        nd.classes, nd.counts = np.zeros(0, np.int32), np.zeros(0, np.int32)
                    else:
                        nd.classes = np.unique(nd.classes % 8).astype(np.int32)
                        nd.counts = rs.randint(1, 3, len(nd.classes)).astype(np.int32)
    ims = rs.randint(0, 256, (2, H, W)).astype(np.uint8)
    got = _check(forests, ims, bins, 0, H)
    assert np.isnan(got[..., 1]).any()


def test_rows_outside_the_range_are_nan():
    H, W, bins = 50, 130, 10
    rs, forests = _random_rows(15, 3, H, n_trees=4, depth=5, C=W * bins, mean_len=20)
    ims = torch.from_numpy(rs.randint(0, 256, (2, H, W)).astype(np.uint8)).cuda()
    tab = hd.HyperDepthForests(forests[10:30], 10, "cuda")
    part = tab.eval(ims, bins, 12, 27).cpu().numpy()
    full = hd.HyperDepthForests(forests, 0, "cuda").eval(ims, bins).cpu().numpy()
    assert np.isnan(part[:, :12]).all() and np.isnan(part[:, 27:]).all()
    assert same_bits(part[:, 12:27], full[:, 12:27])
    assert not np.isnan(full[..., 0]).any()
    with pytest.raises(ValueError, match="forests loaded for"):
        tab.eval(ims, bins, 5, 27)
    assert np.isnan(tab.eval(ims, bins, 20, 20).cpu().numpy()).all()          # an empty range


def test_reuse_and_non_default_stream_give_identical_output():
    H, W, bins = 96, 320, 10
    rs, forests = _random_rows(16, 4, H, n_trees=6, depth=8, C=W * bins, mean_len=64)
    tab = hd.HyperDepthForests(forests, 0, "cuda")
    ims = torch.from_numpy(rs.randint(0, 256, (2, H, W)).astype(np.uint8)).cuda()
    a = tab.eval(ims, bins).cpu().numpy()
    b = tab.eval(ims, bins).cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = torch.full((2, H, W, 3), 7.0, device="cuda")
        c = tab.eval(ims, bins, out=out)
    s.synchronize()
    assert c is out
    c = c.cpu().numpy()
    assert same_bits(a, b) and same_bits(a, c)
    assert same_bits(a, R.eval_rows(forests, 0, ims.cpu().numpy(), bins, 0, H))
