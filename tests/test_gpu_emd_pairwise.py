"""dgv2_emd_pairwise_cost: the all-pairs approximate-matching EMD cost without the match matrix, its host wrapper
(pairwise_emd_cost) and the engine="pairwise" path of compute_cov_mmd_1nna."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
U = 2.0 ** -24   # unit roundoff of fp32


def clouds(seed, B, n, scale=1.0):
    """The recipe of tests/test_gpu_pointcloud.py."""
    return (np.random.default_rng(seed).standard_normal((B, n, 3)) * scale).astype(F32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pair_sets(B1, B2, n, m):
    return clouds(n, B1, n, 0.4), clouds(m + 3, B2, m, 0.4)


# multiR = 3; multiL = 4; exactly one tile; two passes with a ragged tail in both sets; the protocol's size
CASES = [(2, 3, 6, 6), (1, 2, 100, 100), (2, 2, 300, 100), (2, 2, 64, 256), (1, 1, 1024, 1024), (1, 2, 1500, 1100),
         (1, 1, 2048, 2048)]


@pytest.mark.parametrize("B1,B2,n,m", CASES)
def test_parity_with_float64_oracle(B1, B2, n, m):
    """cost[i, j] against matchcost(approxmatch) of the float64 restatement, at the 1e-3 relative that
    test_emd_match_cost_and_gradient holds the device cost to."""
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    from oracle import pointcloud as pc
    a, b = pair_sets(B1, B2, n, m)
    got = pairwise_emd_cost(dev(a), dev(b))
    assert got.shape == (B1, B2) and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = np.zeros((B1, B2))
    for i in range(B1):
        for j in range(B2):
            ai, bj = a[i:i + 1], b[j:j + 1]
            want[i, j] = pc.matchcost(ai, bj, pc.approxmatch(ai, bj))[0]
    print(f"({B1},{B2},{n},{m}): worst relative error {np.abs(got / want - 1).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-3)


def chain_pairwise(n, m):
    """Longest chain of roundings behind one term of the pairwise kernel's sum (include/dgv2.h): a lane adds
    9 levels x ceil(n / 1024) own points x m terms in order, the block sum adds 6 butterfly steps and 16 wave partials;
    each term carries the rounding of its product and of its square root."""
    return 9 * math.ceil(n / 1024) * m + 6 + 16 + 2


def chain_batched(n, m):
    """The same for dgv2_emd_approxmatch + dgv2_emd_matchcost: match[l, k] is a sum over 9 levels; a lane of the cost
    kernel (256 lanes, min(m, 32) chunks of l) adds ceil(n / 256) own points x ceil(m / chunks) terms, the block sum 6
    butterfly steps and 4 wave partials, the atomics one add per chunk; product and square root as above."""
    chunks = min(m, 32)
    return 9 + math.ceil(n / 256) * math.ceil(m / chunks) + 6 + 4 + chunks + 2


@pytest.mark.parametrize("B1,B2,n,m", CASES)
def test_against_the_batched_device_path(B1, B2, n, m):
    """Both paths sum non-negative terms from the same matching arithmetic, so each is within (its longest chain) x 2^-24
    relative of the exact sum of its terms: the two may differ by the sum of the two bounds."""
    from gans.metrics.distance import earth_mover_distance
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    a, b = pair_sets(B1, B2, n, m)
    ta, tb = dev(a), dev(b)
    got = pairwise_emd_cost(ta, tb).cpu().double()
    want = torch.stack([earth_mover_distance(ta[i:i + 1].expand(B2, -1, -1).contiguous(), tb) for i in range(B1)])
    want = want.cpu().double()
    bound = (chain_pairwise(n, m) + chain_batched(n, m)) * U
    worst = float(((got - want).abs() / want).max())
    print(f"({B1},{B2},{n},{m}): worst relative difference {worst:.3e}, bound {bound:.3e}, ratio {worst / bound:.3f}")
    assert worst <= bound


def test_position_independent_and_repeatable():
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    a, b = pair_sets(3, 4, 300, 300)
    ta, tb = dev(a), dev(b)
    full = pairwise_emd_cost(ta, tb)
    assert torch.equal(full, pairwise_emd_cost(ta, tb))
    for i in range(3):
        for j in range(4):
            one = pairwise_emd_cost(ta[i:i + 1].contiguous(), tb[j:j + 1].contiguous())
            assert torch.equal(one[0, 0], full[i, j]), (i, j)


def test_a_matrix_launched_in_slabs_of_rows_is_the_same_matrix():
    """More pairs than one launch takes (the wrapper walks the rows in slabs): the same bits as row blocks of another
    size, each of which is one launch."""
    from gans.metrics.distance.emd.earth_mover_distance import PAIRS_PER_LAUNCH, pairwise_emd_cost
    B1, B2 = 2 * PAIRS_PER_LAUNCH // 100 + 7, 100
    a, b = clouds(5, B1, 3, 0.4), clouds(6, B2, 2, 0.4)
    ta, tb = dev(a), dev(b)
    assert B1 * B2 > 2 * PAIRS_PER_LAUNCH
    full = pairwise_emd_cost(ta, tb)
    assert full.shape == (B1, B2)
    parts = torch.cat([pairwise_emd_cost(ta[i:i + 50], tb) for i in range(0, B1, 50)])
    assert torch.equal(full, parts)
    assert bool(torch.isfinite(full).all()) and float(full.min()) > 0


def test_no_match_matrix_is_allocated():
    """8 x 8 pairs at 2048 + 2048 points: the peak rises by less than one pair's match (16 MB); the batched path
    allocates 8 of them for one row."""
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    a, b = pair_sets(8, 8, 2048, 2048)
    ta, tb = dev(a), dev(b)
    pairwise_emd_cost(ta[:1], tb[:1])   # anything lazily initialised is initialised
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    cost = pairwise_emd_cost(ta, tb)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < 2048 * 2048 * 4, rise
    assert bool(torch.isfinite(cost).all()) and float(cost.min()) > 0


def test_above_the_cap_the_entry_declines_and_the_wrapper_falls_back():
    import dgv2_native as N
    from gans.metrics.distance import earth_mover_distance
    from gans.metrics.distance.emd.earth_mover_distance import PAIR_MAX_POINTS, pairwise_emd_cost
    n = PAIR_MAX_POINTS // 2
    a, b = pair_sets(1, 1, n + 1, n)
    ta, tb = dev(a), dev(b)
    cost = torch.full((1, 1), -1.0, device=DEV)
    rc = N.lib.dgv2_emd_pairwise_cost(N.ptr(cost), N.ptr(ta), N.ptr(tb), 1, 1, n + 1, n, N.stream())
    torch.cuda.synchronize()
    assert rc != 0 and float(cost) == -1.0
    assert N.lib.dgv2_emd_pairwise_cost(None, N.ptr(ta), N.ptr(tb), 1, 1, 8, 8, N.stream()) != 0
    assert N.lib.dgv2_emd_pairwise_cost(N.ptr(cost), N.ptr(ta), N.ptr(tb), 1, 1, 0, 8, N.stream()) != 0
    got = pairwise_emd_cost(ta, tb)   # the same two kernels as the batched path: apart by the order of its atomics at most
    want = earth_mover_distance(ta, tb)
    assert got.shape == (1, 1)
    assert abs(float(got) - float(want)) <= 2 * chain_batched(n + 1, n) * U * float(want)


def test_rejects_what_shapes_rejects():
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    ok = torch.zeros(2, 4, 3, device=DEV)
    with pytest.raises(RuntimeError):
        pairwise_emd_cost(torch.zeros(2, 4, 3), torch.zeros(2, 4, 3))                  # CPU tensors
    with pytest.raises(RuntimeError):
        pairwise_emd_cost(ok.double(), ok.double())
    with pytest.raises(RuntimeError):
        pairwise_emd_cost(ok, torch.zeros(2, 4, 2, device=DEV))
    with pytest.raises(RuntimeError):
        pairwise_emd_cost(ok.transpose(0, 1), ok)                                      # not contiguous


def test_one_point_against_one_point():
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    a, b = clouds(1, 3, 1, 0.4), clouds(2, 2, 1, 0.4)
    got = pairwise_emd_cost(dev(a), dev(b)).cpu().numpy()
    want = np.linalg.norm(a.astype(np.float64)[:, None, 0, :] - b.astype(np.float64)[None, :, 0, :], axis=-1)
    np.testing.assert_allclose(got, want, rtol=1e-6)


def test_cov_mmd_1nna_engines():
    """The sets of test_cov_mmd_1nna_on_two_small_sets: engine="pairwise" has the keys of "batched" and its EMD
    statistics within that test's 2e-3; the default engine is the batched one, unchanged.

    dgv2_emd_matchcost adds its min(m, 32) chunk sums with float atomics, so two runs of the batched path itself may
    differ in the last bits of an EMD (seen: mmd-emd 0.28485047817 / 0.28485050797).  "Default == batched, identical
    dicts" is therefore asked twice: of the real kernels with every key identical but the two EMD means, which may be
    apart by the reordering of those chunk sums at most; and of the whole dict, bit for bit, with the batched EMD
    replaced by a function that returns the same bits every time."""
    import gans.metrics.cov_mmd_1nna as C
    from gans.metrics.cov_mmd_1nna import compute_cov_mmd_1nna
    from gans.metrics.distance.emd.earth_mover_distance import pairwise_emd_cost
    gen, ref = clouds(41, 6, 128, 0.3), clouds(42, 5, 128, 0.3) + F32(0.1)
    kw = dict(batch_size=4, metrics=("cd", "emd", "dcd"), verbose=False)
    default = compute_cov_mmd_1nna(dev(gen), dev(ref), **kw)
    batched = compute_cov_mmd_1nna(dev(gen), dev(ref), engine="batched", **kw)
    pairwise = compute_cov_mmd_1nna(dev(gen), dev(ref), engine="pairwise", **kw)
    assert set(default) == set(batched)
    atomics = 2 * 32 * U                                                  # two orders of at most 32 chunk sums
    for k in batched:
        if k in ("mmd-emd", "mmd-sample-emd"):
            assert abs(default[k] - batched[k]) <= atomics * abs(batched[k]), k
        else:
            assert default[k] == batched[k], k

    def repeatable_emd(lhs, chunk):                                       # lhs: copies of one cloud (_pairwise_distance)
        return pairwise_emd_cost(lhs[:1].contiguous(), chunk)[0] / float(lhs.size(1))
    real = C._DIST["emd"]
    C._DIST["emd"] = repeatable_emd
    try:
        assert compute_cov_mmd_1nna(dev(gen), dev(ref), **kw) == compute_cov_mmd_1nna(dev(gen), dev(ref), engine="batched", **kw)
    finally:
        C._DIST["emd"] = real
    assert set(pairwise) == set(batched)
    for k in ("mmd-emd", "mmd-sample-emd"):
        assert abs(pairwise[k] - batched[k]) <= 2e-3 * abs(batched[k]), k
    for k in batched:                                                     # cd / dcd stay on the batched path
        if k.endswith("-cd") or k.endswith("-dcd"):
            assert pairwise[k] == batched[k], k
    with pytest.raises(ValueError):
        compute_cov_mmd_1nna(dev(gen), dev(ref), engine="fastest", **kw)
