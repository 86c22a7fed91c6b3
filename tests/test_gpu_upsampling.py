"""Beam upsampling on the GPU: dgv2_depth_score and dgv2_beam_split (csrc/upsample.hip) against the CPU restatements of
tests/upsampling_ref.py and the fixture of the reference's own depth.py, then gans/upsampling.py and eval_upsampling.py
end to end on the toy checkpoint.

Tolerances.  Columns 0 - 2 and 4 - 7 of depth_score are float64 sums of float32 terms that the CPU restatement computes
with the same separately rounded operations, so the only difference is the order of the float64 sum: rtol = n 2^-52, the
reordering bound of a sum of n non-negative terms; columns 4 - 7 are sums of mask values and must be equal.  Column 3
holds logf, whose last bit is the library's: it is held, through depth_summary, to the rtol = 1e-5 that
test_gpu_metrics.py::test_depth_summaries gives the tensor-op port, against the reference's fixture and against a
float64 oracle.  A single-pixel image is held to atol = 1e-6 on rmse_log instead: there the difference of two float32
logarithms is the whole value, and it cancels in the reference itself.  beam_split is compared exactly.

Measured on an MI355X: columns 0 - 2 at most 3.0e-16 relative from the restatement (bounds
7.8e-15 .. 7.3e-12), columns 4 - 7 equal, the summaries within 6.9e-8 of the float64 oracle; the file runs in about 5 s,
2 s of it the profiler's first use.

The end-to-end part is not a test of reconstruction quality: eight steps on a 16 x 64 toy generator prove nothing about
it, and no number for it is claimed."""
import json
import os

import numpy as np
import pytest
import torch

import upsampling_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = list(zip(R.SEEDS, R.SHAPES))
SPLITS = ((16, 64, 4, 0), (16, 64, 4, 3), (7, 5, 3, 1), (6, 3, 1, 0), (5, 4, 5, 2))       # (H, W, factor, offset)
EXACT, COUNTS = (0, 1, 2, 4, 5, 6, 7), (4, 5, 6, 7)


def native():
    from gans.models.ops import native as n
    return n


def score(ref, gen, mask=None):
    out = native().depth_score(ref.to(DEV), gen.to(DEV), None if mask is None else mask.to(DEV))
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(ref), 8) and not out.requires_grad
    return out.cpu()


_refs = {}


def case(seed, shape):
    """Inputs and both CPU references of one seeded case, computed once."""
    if (seed, shape) not in _refs:
        ref, gen, mask = R.make_inputs(seed, shape)
        _refs[(seed, shape)] = {"in": (ref, gen, mask), "f32": R.score_sums_f32(ref, gen, mask),
                                "f64": R.summary_f64(ref, gen, mask), "margin": R.threshold_margin(ref, gen)}
    return _refs[(seed, shape)]


def assert_obeys_restatement(got, want, n, what):
    rtol = n * 2.0 ** -52
    for c in EXACT:
        err = float(((got[:, c] - want[:, c]).abs() / want[:, c].abs().clamp_min(1e-300)).max())
        print(f"{what} column {c}: relative difference {err:.2e} (bound {rtol:.2e})")
    for c in COUNTS:
        np.testing.assert_array_equal(got[:, c].numpy(), want[:, c].numpy(), err_msg=f"{what} column {c}")
    for c in (0, 1, 2):
        np.testing.assert_allclose(got[:, c].numpy(), want[:, c].numpy(), rtol=rtol, atol=0, err_msg=f"{what} column {c}")


# ---------------------------------------------------------------------------------------
# 1. depth_score
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape", CASES)
def test_score_exact_columns_obey_the_float32_restatement(seed, shape):
    c = case(seed, shape)
    assert c["margin"] > 1e-6, "a pixel sits on a threshold: the accuracy columns would depend on the last bit"
    n = int(np.prod(shape[1:]))
    assert_obeys_restatement(score(*c["in"]), c["f32"], n, f"seed {seed} {shape}")


@pytest.mark.parametrize("seed,shape", CASES)
def test_score_summaries_against_the_float64_oracle(seed, shape):
    c = case(seed, shape)
    assert c["margin"] > 1e-6
    got = native().depth_summary(score(*c["in"]))
    for k in R.KEYS:
        err = float(((got[k] - c["f64"][k]).abs() / c["f64"][k].abs()).max())
        print(f"seed {seed} {shape} {k}: relative error {err:.2e}")
        np.testing.assert_allclose(got[k].numpy(), c["f64"][k].numpy(), rtol=1e-5, atol=0, err_msg=k)


def test_score_summaries_against_the_reference_fixture():
    d = np.load(os.path.join(GOLDEN, "metrics.npz"))
    ref, gen, mask = (torch.from_numpy(d[k]) for k in ("depth_ref", "depth_gen", "depth_mask"))
    got = native().depth_summary(score(ref, gen, mask))
    assert tuple(got) == R.KEYS
    for k in R.KEYS:
        assert got[k].dtype == torch.float64
        np.testing.assert_allclose(got[k].numpy(), d["depth_" + k], rtol=1e-5, atol=0, err_msg=k)
    same = native().depth_summary(score(ref, ref))
    assert float(same["rmse"].abs().max()) == 0 and float(same["rmse_log"].abs().max()) == 0
    assert float(same["accuracy_1"].min()) == 1.0


def test_score_single_pixel_images():
    ref = torch.tensor([8.0, 20.0, 50.0, 1.5]).reshape(4, 1, 1, 1)
    gen = torch.tensor([8.5, 15.0, 51.0, 4.0]).reshape(4, 1, 1, 1)
    assert R.threshold_margin(ref, gen) > 1e-6
    got, want = native().depth_summary(score(ref, gen)), R.summary_f64(ref, gen)
    for k in R.KEYS:
        tol = dict(rtol=0, atol=1e-6) if k == "rmse_log" else dict(rtol=1e-5, atol=0)
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), err_msg=k, **tol)


def test_score_without_a_mask_is_a_mask_of_ones():
    ref, gen, _ = case(*CASES[1])["in"]
    assert torch.equal(score(ref, gen), score(ref, gen, torch.ones_like(ref)))


def test_score_skips_masked_pixels():
    """An all-zero mask gives a zero row and a NaN summary, whatever the masked pixels hold: 0 / 0, a zero depth."""
    ref, gen, mask = (t.clone() for t in case(*CASES[0])["in"])
    want = R.score_sums_f32(ref, gen, mask)
    mask[0] = 0.0
    ref[0, 0, 0, :3] = 0.0
    gen[0] = 0.0
    gen[1][mask[1] == 0] = float("nan")
    got = score(ref, gen, mask)
    assert torch.equal(got[0], torch.zeros(8, dtype=torch.float64))
    assert all(bool(torch.isnan(v[0])) for v in native().depth_summary(got).values())
    assert_obeys_restatement(got[1:], want[1:], 35, "beside a fully masked image")


def test_score_takes_the_mask_as_a_weight():
    ref, gen, mask = case(*CASES[3])["in"]
    weight = mask * 0.5 + 0.5 * (torch.rand(mask.shape, generator=torch.Generator().manual_seed(7)) > 0.5).float() * mask
    assert set(weight.unique().tolist()) == {0.0, 0.5, 1.0}
    assert_obeys_restatement(score(ref, gen, weight), R.score_sums_f32(ref, gen, weight), 3 * 43, "half weights")


def test_score_bits_do_not_depend_on_the_batch_or_the_run():
    """n = 5123: some threads own two groups, three pixels are left over, and image 1 of a batch starts at an address
    that is not 16-byte aligned while the same image alone does."""
    ref, gen, mask = R.make_inputs(105, (3, 1, 47, 109))
    batch = score(ref, gen, mask)
    assert torch.equal(batch, score(ref, gen, mask))
    assert torch.equal(batch[1:2], score(ref[1:2].contiguous(), gen[1:2].contiguous(), mask[1:2].contiguous()))
    assert torch.equal(batch.flip(0), score(ref.flip(0).contiguous(), gen.flip(0).contiguous(), mask.flip(0).contiguous()))
    assert_obeys_restatement(batch, R.score_sums_f32(ref, gen, mask), 5123, "n = 5123")


@pytest.mark.parametrize("n", (35, 129, 1024))
def test_score_load_paths_give_the_same_bits(n):
    N = native()
    ref, gen, mask = (t.reshape(1, n + 1).to(DEV) for t in R.make_inputs(200 + n, (1, 1, 1, n + 1)))
    views = [t[:, 1:] for t in (ref, gen, mask)]
    assert all(v.is_contiguous() and v.data_ptr() % 16 == 4 for v in views)
    copies = [v.clone() for v in views]
    assert all(c.data_ptr() % 16 == 0 for c in copies)
    shifted, aligned = N.depth_score(*views), N.depth_score(*copies)
    assert torch.equal(shifted, aligned)
    assert torch.equal(N.depth_score(copies[0], views[1], copies[2]), aligned)       # one misaligned array is enough
    assert torch.equal(N.depth_score(views[0], views[1]), N.depth_score(copies[0], copies[1]))
    assert_obeys_restatement(aligned.cpu(), R.score_sums_f32(*[c.cpu() for c in copies]), n, f"n = {n}")


def test_score_rejections_launch_nothing():
    import dgv2_native as N
    ref, gen, mask = (t.to(DEV) for t in case(*CASES[0])["in"])
    sums = torch.full((3, 8), 7.0, device=DEV, dtype=torch.float64)

    def call(ptrs=None, B=3, n=35):
        p = dict(sums=sums.data_ptr(), ref=ref.data_ptr(), gen=gen.data_ptr(), mask=mask.data_ptr())
        p.update(ptrs or {})
        return N.lib.dgv2_depth_score(p["sums"], p["ref"], p["gen"], p["mask"], B, n, N.stream())
    rcs = {"B=0": call(B=0), "n=0": call(n=0), "n=2^31": call(n=2 ** 31),
           **{f"null {k}": call({k: None}) for k in ("sums", "ref", "gen")}}
    torch.cuda.synchronize()
    assert all(rc == N.EINVAL for rc in rcs.values()), rcs
    assert float(sums.min()) == 7.0 and float(sums.max()) == 7.0
    assert call({"mask": None}) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums.cpu(), score(ref.cpu(), gen.cpu()))


def _count(fn):
    from test_gpu_sim2real import _count as count
    return count(fn)


def test_score_is_one_launch():
    N = native()
    ref, gen, mask = (t.to(DEV) for t in case(*CASES[2])["in"])
    N.depth_score(ref, gen, mask)
    names, launches = _count(lambda: N.depth_score(ref, gen, mask))
    assert names == ["dgv2_depth_score"] and launches == 1, (names, launches)


# ---------------------------------------------------------------------------------------
# 2. beam_split
# ---------------------------------------------------------------------------------------
def split(depth, valid, factor, offset, mode):
    out = native().beam_split(depth.to(DEV), None if valid is None else valid.to(DEV), factor, offset, mode)
    assert all(v.dtype == torch.float32 and v.shape == depth.shape and not v.requires_grad for v in out.values())
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("H,W,factor,offset", SPLITS)
def test_split_equals_the_restatement(H, W, factor, offset):
    depth, valid = R.make_scan(300 + H + factor, 2, H, W, factor, offset)
    share = float((valid == 0).float().mean())
    assert 0.2 < share < 0.6 and bool((valid[:, :, offset::factor, 1 % W] == 0).all())
    for mode in ("nearest", "linear"):
        got, want = split(depth, valid, factor, offset, mode), R.beam_split_ref(depth, valid, factor, offset, mode)
        assert set(got) == {"recon", "recon_mask", "obs", "held"}
        for k in want:
            np.testing.assert_array_equal(got[k].numpy(), want[k].numpy(), err_msg=f"{mode} {k}")
        # what the outputs promise each other
        v = (valid != 0).float()
        assert torch.equal(got["obs"] + got["held"], v)
        seen = got["obs"] == 1
        assert torch.equal(got["recon"][seen], depth[seen]) and bool((got["recon_mask"][seen] == 1).all())
        assert float(got["recon"][:, :, :, 1 % W].abs().max()) == 0 and float(got["recon_mask"][:, :, :, 1 % W].max()) == 0
        assert bool((got["recon"][got["recon_mask"] == 0] == 0).all())
        if factor == 1:
            assert torch.equal(got["recon"], depth * v) and float(got["held"].max()) == 0
    none = split(depth, valid, factor, offset, "none")
    assert set(none) == {"obs", "held"}
    assert torch.equal(none["obs"], want["obs"]) and torch.equal(none["held"], want["held"])


def test_split_mode_0_takes_null_reconstruction_pointers():
    import dgv2_native as N
    H, W, factor, offset = SPLITS[2]
    depth, valid = (t.to(DEV) for t in R.make_scan(1, 2, H, W, factor, offset))
    obs, held = torch.full_like(depth, 7.0), torch.full_like(depth, 7.0)
    recon = torch.full_like(depth, 7.0)
    args = (depth.data_ptr(), valid.data_ptr(), 2, H, W, factor, offset)
    assert N.lib.dgv2_beam_split(None, recon.data_ptr(), obs.data_ptr(), held.data_ptr(), *args, 1, N.stream()) == N.EINVAL
    assert N.lib.dgv2_beam_split(recon.data_ptr(), recon.data_ptr(), obs.data_ptr(), None, *args, 0, N.stream()) == N.EINVAL
    torch.cuda.synchronize()
    assert float(obs.min()) == 7.0 and float(held.min()) == 7.0
    assert N.lib.dgv2_beam_split(recon.data_ptr(), recon.data_ptr(), obs.data_ptr(), held.data_ptr(), *args, 0, N.stream()) == 0
    torch.cuda.synchronize()
    assert float(recon.min()) == 7.0 and float(recon.max()) == 7.0           # mode 0 writes the two masks only
    first = (obs.clone(), held.clone())
    assert N.lib.dgv2_beam_split(None, None, obs.data_ptr(), held.data_ptr(), *args, 0, N.stream()) == 0
    torch.cuda.synchronize()
    want = R.beam_split_ref(depth.cpu(), valid.cpu(), factor, offset, "none")
    assert torch.equal(obs.cpu(), want["obs"]) and torch.equal(held.cpu(), want["held"])
    assert torch.equal(first[0], obs) and torch.equal(first[1], held)


def test_split_without_valid_is_all_valid_and_repeats():
    H, W, factor, offset = SPLITS[1]
    depth, _ = R.make_scan(2, 2, H, W, factor, offset)
    for mode in ("nearest", "linear"):
        a, b = split(depth, None, factor, offset, mode), split(depth, torch.ones_like(depth), factor, offset, mode)
        again = split(depth, None, factor, offset, mode)
        want = R.beam_split_ref(depth, None, factor, offset, mode)
        for k in want:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], again[k]) and torch.equal(a[k], want[k]), (mode, k)
        assert float(a["recon_mask"].min()) == 1


def test_split_is_one_launch():
    N = native()
    depth, valid = (t.to(DEV) for t in R.make_scan(3, 2, 16, 64, 4, 0))
    for mode in ("none", "linear"):
        N.beam_split(depth, valid, 4, 0, mode)
        names, launches = _count(lambda: N.beam_split(depth, valid, 4, 0, mode))
        assert names == ["dgv2_beam_split"] and launches == 1, (mode, names, launches)


# ---------------------------------------------------------------------------------------
# 3. end to end on the toy checkpoint
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLDEN, "inversion.npz"))
    return {k: d[k] for k in d.files if k.startswith("invert.") or k == "angle_file"}


@pytest.fixture(scope="module")
def fitter(gold):
    from gans.coords import CoordBridge
    from gans.models.builder import build_generator
    from gans.pretrained import autoload_ckpt
    from test_gpu_sim2real import make_fitter
    coord = CoordBridge(16, 64, 1.45, 80.0, angle_array=gold["angle_file"]).to(DEV)
    ck = autoload_ckpt(os.path.join(GOLDEN, "checkpoint_small.pth"))
    cfg = ck["cfg"].model.generator
    cfg.synthesis_kwargs.num_fp16_layers = 0
    G = build_generator(cfg)
    G.load_state_dict(ck["G_ema"])
    return make_fitter(G.eval().to(DEV), coord, gold, 8, False)


class Spy:
    """The fitter as upsample_scans sees it, keeping what it was given and what it answered."""

    def __init__(self, fitter):
        self.fitter, self.coord, self.calls = fitter, fitter.coord, []

    def fit(self, depth, mask):
        out = self.fitter.fit(depth, mask)
        self.calls.append((depth.clone(), mask.clone(), {k: v.clone() for k, v in out.items()}))
        return out


def scans(gold):
    return tuple(torch.from_numpy(gold[k]).to(DEV).float().contiguous() for k in ("invert.depth", "invert.mask"))


def test_gan_method_is_the_fit_converted_by_hand(gold, fitter):
    from gans.upsampling import upsample_scans
    N = native()
    depth, valid = scans(gold)
    spy = Spy(fitter)
    got = upsample_scans(depth, valid, factor=4, method="gan", fitter=spy)
    assert len(spy.calls) == 1 and set(got) == {"depth", "mask", "obs", "held"}
    d_in, m_in, out = spy.calls[0]
    masks = N.beam_split(depth, valid, 4, 0, "none")
    assert torch.equal(got["obs"], masks["obs"]) and torch.equal(got["held"], masks["held"])
    assert torch.equal(m_in, masks["obs"]) and torch.equal(d_in, depth * masks["obs"])
    coord = fitter.coord
    by_hand = coord.convert(coord.convert(out["inv_depth_orig"], "inv_depth_norm", "depth_norm"), "depth_norm", "depth")
    assert torch.equal(got["depth"], by_hand) and torch.equal(got["mask"], (out["raydrop_prob"] >= 0.5).float())
    assert tuple(got["depth"].shape) == (2, 1, 16, 64) and not got["depth"].requires_grad


def test_benchmark_over_the_three_methods(gold, fitter):
    from gans.upsampling import UpsamplingBenchmark
    N = native()
    depth, valid = scans(gold)
    bench = UpsamplingBenchmark(("nearest", "linear", "gan"), factor=4, offset=0)
    bench.update(depth, valid, fitter=fitter)
    bench.update(depth.flip(0).contiguous(), valid.flip(0).contiguous(), fitter=fitter)
    s = bench.summary()
    assert tuple(s) == ("nearest", "linear", "gan")
    for method, r in s.items():
        assert set(r["per_scan"]) == set(R.KEYS) == set(r["pooled"]) and r["scans"] == r["scored_scans"] == 4
        assert all(np.isfinite(v) for v in list(r["per_scan"].values()) + list(r["pooled"].values())), (method, r)
        assert 0.0 <= r["coverage"] <= 1.0 and r["pixels"] == 2 * float(N.beam_split(depth, valid, 4, 0)["held"].sum())
    for method in ("nearest", "linear"):
        sp = N.beam_split(depth, valid, 4, 0, method)
        sums = N.depth_score(depth, sp["recon"], sp["held"])
        per_scan = {k: float(v.mean()) for k, v in N.depth_summary(sums).items()}
        pooled = {k: float(v) for k, v in N.depth_summary(sums.sum(dim=0)).items()}
        for k in R.KEYS:      # both batches hold the same two scans
            assert s[method]["per_scan"][k] == pytest.approx(per_scan[k], rel=1e-12), (method, k)
            assert s[method]["pooled"][k] == pytest.approx(pooled[k], rel=1e-12), (method, k)
        covered, held = (sp["held"] * sp["recon_mask"]).double().sum(), sp["held"].double().sum()
        assert s[method]["coverage"] == pytest.approx(float(covered / held), rel=1e-12)


def test_command_line_on_synthetic_scans(capsys, tmp_path):
    import eval_upsampling
    out = tmp_path / "scores.json"
    eval_upsampling.main(["--synthetic", "4", "--methods", "nearest,linear", "--factor", "4", "--batch_size", "3",
                          "--out", str(out)])
    lines = capsys.readouterr().out.strip().splitlines()
    res = json.loads(lines[-1], parse_constant=lambda c: pytest.fail(f"not strict JSON: {c}"))
    assert [ln for ln in lines[:-1] if ln.startswith("[")] and lines[-2].startswith("[4/4]")
    assert json.loads(out.read_text()) == res
    assert tuple(res["methods"]) == ("nearest", "linear") and res["scans"] == 4 and res["captured"] is False
    assert res["scans_per_second"] > 0 and res["args"]["factor"] == 4 and res["args"]["methods"] == ["nearest", "linear"]
    for r in res["methods"].values():
        assert set(r["per_scan"]) == set(R.KEYS) == set(r["pooled"])
        assert all(v is not None and np.isfinite(v) for v in list(r["per_scan"].values()) + list(r["pooled"].values()))
