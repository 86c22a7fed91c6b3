"""GPU checks of the segmentation training step: the three entries of csrc/sgd.hip and
native.fused_clip_sgd_step against float64, their repeatability, the loss scale, and semseg.trainer.Trainer -- step,
validation, checkpoint and the command line.

Bounds (set by the arithmetic, section 34.2):
  norm      |sc[0] - norm64| <= 2^-18 norm64: at most 3 x 4 chained fused multiply-adds per thread and 8 reduce levels
            in fp32, under 32 roundings of 2^-24; the partials are then added in double.
  factor    |sc[1] - factor64| <= (2^-18 + 2^-23) factor64: the norm's error, one division, one rounding to fp32.
  elements  |m - m64| <= 8 * 2^-24 (momentum |m_prev| + |d64|),  |p - p64| <= 8 * 2^-24 (|p64| + lr |m64|), where the
            float64 values follow  d = f g + wd p;  m = momentum m_prev + d;  p -= lr m  from the SAME fp32 inputs the
            kernel read: the tensors, the fp32-rounded lr / momentum / weight decay, and f = sc[1], the fp32 factor the
            kernel itself read from memory.  Each is a chain of at most five fp32 operations.
"""
import copy
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 16385, 147456] + [7] * 64     # 74 tensors: two chunks of the 72-tensor launch
OFF_ALL, OFF_G = 8, 6          # tensor 8: p, g and m start one element into their buffers; tensor 6: only g does
CASES = [(0.9, 1e-4, 1.0), (0.0, 0.0, 1.0), (0.9, 1e-4, 1e9), (0.9, 0.0, 0.0)]     # (momentum, weight decay, max_norm)
LR = 0.05
G_SCALE = 0.05                 # |g| ~ 0.05 * sqrt(166k / 3) ~ 12: max_norm = 1 clips, 1e9 does not


def hash_unit(plane, index, n):
    """n reproducible values in [-1, 1) from an integer mix of (plane, index, position)."""
    z = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(plane * 1000003 + index * 7919 + 12345)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


@pytest.fixture(scope="module")
def base():
    """Host values shared by the optimizer tests, never modified: parameters, momentum buffers, two gradient sets."""
    return {"p": [hash_unit(0, i, n) for i, n in enumerate(LENGTHS)],
            "m": [hash_unit(1, i, n) * np.float32(0.1) for i, n in enumerate(LENGTHS)],
            "g": [[hash_unit(2 + s, i, n) * np.float32(G_SCALE) for i, n in enumerate(LENGTHS)] for s in range(3)]}


def place(arrs, offset_at=()):
    """Device copies; tensors named in offset_at are views starting one element (4 bytes) into a larger buffer."""
    out = []
    for i, a in enumerate(arrs):
        if i in offset_at:
            buf = torch.zeros(a.size + 5, device=DEV)
            t = buf[1:1 + a.size]
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.from_numpy(a).to(DEV)
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


def run_entries(ps, gs, ms, lr, momentum, wd, max_norm, scale_state=None, growth_interval=2000):
    """One step through the C ABI entries alone, 72 tensors per launch.  -> sc (fp32 [4])."""
    import dgv2_native as N

    parts = torch.full((len(ps), N.SUMSQ_PARTS), float("nan"), device=DEV)
    sc = torch.full((4,), float("nan"), device=DEV)
    n_all = [p.numel() for p in ps]
    for i in range(0, len(ps), 72):
        g = gs[i:i + 72]
        N.call("dgv2_sumsq_list", N.ptr_array(g), N.int_array(n_all[i:i + 72]), len(g), parts[i:].data_ptr(), N.stream())
    N.call("dgv2_clip_prep", N.ptr(parts), parts.numel(), max_norm, N.ptr(scale_state), 2.0, 0.5, growth_interval, N.ptr(sc),
           N.stream())
    for i in range(0, len(ps), 72):
        p, g = ps[i:i + 72], gs[i:i + 72]
        m = ms[i:i + 72] if ms is not None else [None] * len(p)
        N.call("dgv2_sgd_step", N.ptr_array(p), N.ptr_array(g), N.ptr_array(m), N.int_array(n_all[i:i + 72]), len(p),
               N.ptr(sc), lr, momentum, wd, N.stream())
    return sc


def f32(x):
    return float(np.float32(x))


def check_scalars(sc, grads, max_norm, scale=1.0):
    """sc[0] and sc[1] against float64 from the fp32 gradients.  -> (norm error, factor error), relative."""
    sc = sc.double().cpu()
    total = sum(float((g.double() ** 2).sum()) for g in grads)
    norm64 = total ** 0.5 / scale
    coef = min(1.0, f32(max_norm) / (norm64 + 1e-6)) if max_norm > 0 else 1.0
    factor64 = coef / scale
    e_norm = abs(float(sc[0]) - norm64) / norm64
    e_fac = abs(float(sc[1]) - factor64) / factor64
    assert e_norm <= 2.0 ** -18, (float(sc[0]), norm64)
    assert e_fac <= 2.0 ** -18 + 2.0 ** -23, (float(sc[1]), factor64)
    return e_norm, e_fac


def check_update(p_old, m_old, g, p_new, m_new, f, lr, momentum, wd):
    """One tensor against the float64 update from the same fp32 inputs (module docstring).  m_old None: zeros;
    momentum 0: m is not compared.  -> the largest error / bound ratios (m, p)."""
    p_old, g, p_new = (t.detach().double().cpu() for t in (p_old, g, p_new))
    m_old = torch.zeros_like(p_old) if m_old is None else m_old.detach().double().cpu()
    lr, mu, wd = f32(lr), f32(momentum), f32(wd)
    d = f * g + wd * p_old
    m64 = mu * m_old + d
    p64 = p_old - lr * m64
    tol_m = 8 * EPS * (mu * m_old.abs() + d.abs())
    tol_p = 8 * EPS * (p64.abs() + lr * m64.abs())
    err_p = (p_new - p64).abs()
    assert bool((err_p <= tol_p).all()), float((err_p / tol_p.clamp_min(1e-300)).max())
    r_m = 0.0
    if momentum != 0:
        err_m = (m_new.detach().double().cpu() - m64).abs()
        assert bool((err_m <= tol_m).all()), float((err_m / tol_m.clamp_min(1e-300)).max())
        r_m = float((err_m / tol_m.clamp_min(1e-300)).max())
    return r_m, float((err_p / tol_p.clamp_min(1e-300)).max())


def snapshot(ts):
    return [None if t is None else t.detach().clone() for t in ts]


# ---------------------------------------------------------------------------------------------------------------------
# 6. the entries against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum, wd, max_norm", CASES)
def test_entries_match_float64(base, momentum, wd, max_norm):
    ps = place(base["p"], (OFF_ALL,))
    ms = place(base["m"], (OFF_ALL,)) if momentum != 0 else None
    worst = [0.0, 0.0, 0.0, 0.0]
    for s in range(2):
        gs = place(base["g"][s], (OFF_ALL, OFF_G))
        g_before = snapshot(gs)
        p_old, m_old = snapshot(ps), (snapshot(ms) if ms is not None else [None] * len(ps))
        sc = run_entries(ps, gs, ms, LR, momentum, wd, max_norm)
        torch.cuda.synchronize()
        assert float(sc[2]) == 0 and float(sc[3]) == 1
        e_norm, e_fac = check_scalars(sc, g_before, max_norm)
        clipped = float(sc[1]) < 1
        assert clipped == (max_norm == 1.0), (float(sc[0]), float(sc[1]))
        f = float(sc[1].double())
        for i in range(len(ps)):
            assert torch.equal(gs[i], g_before[i]), f"gradient {i} was modified"
            r_m, r_p = check_update(p_old[i], m_old[i], gs[i], ps[i], None if ms is None else ms[i], f, LR, momentum, wd)
            worst = [max(worst[0], e_norm), max(worst[1], e_fac), max(worst[2], r_m), max(worst[3], r_p)]
    print(f"\n[sgd entries] case {(momentum, wd, max_norm)}: norm rel err {worst[0]:.3e} (bound {2.0 ** -18:.3e}), factor rel err "
          f"{worst[1]:.3e}, worst m err / bound {worst[2]:.3f}, worst p err / bound {worst[3]:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the same cases through fused_clip_sgd_step on a torch.optim.SGD
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum, wd, max_norm", CASES)
def test_fused_step_on_torch_sgd(base, momentum, wd, max_norm):
    from gans.models.ops.native import fused_clip_sgd_step

    params = [torch.nn.Parameter(t) for t in place(base["p"], (OFF_ALL,))]
    opt = torch.optim.SGD(params, lr=LR, momentum=momentum, weight_decay=wd)
    for s in range(2):
        for p, g in zip(params, place(base["g"][s], (OFF_ALL, OFF_G))):
            p.grad = g
        p_old = snapshot(params)
        m_old = [opt.state[p].get("momentum_buffer") for p in params]
        m_old = snapshot(m_old)
        sc = fused_clip_sgd_step(opt, max_norm)
        check_scalars(sc, [p.grad for p in params], max_norm)
        f = float(sc[1].double())
        for i, p in enumerate(params):
            m_new = opt.state[p]["momentum_buffer"] if momentum != 0 else None
            check_update(p_old[i], m_old[i], p.grad, p, m_new, f, LR, momentum, wd)
    if momentum != 0:
        assert all(opt.state[p]["momentum_buffer"].shape == p.shape for p in params)
    else:
        assert all("momentum_buffer" not in opt.state[p] or opt.state[p]["momentum_buffer"] is None for p in params)

    # the state is torch's: a fresh torch SGD adopts it, and its own third step (torch's fp32 norm, clip and chain)
    # matches a third fused step within the bound of test 6 -- against the float64 update and against the fused values.
    # Measured: torch's worst error / bound 0.40 (p) and 0.35 (m) over the four cases.
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    fresh = torch.optim.SGD(twins, lr=LR, momentum=momentum, weight_decay=wd)
    fresh.load_state_dict(copy.deepcopy(opt.state_dict()))      # load_state_dict may keep the very tensors it is given
    g3 = place(base["g"][2], (OFF_ALL, OFF_G))
    for p, t, g in zip(params, twins, g3):
        p.grad = g
        t.grad = g.clone()
    p_old = snapshot(params)
    m_old = snapshot([opt.state[p].get("momentum_buffer") for p in params])
    sc = fused_clip_sgd_step(opt, max_norm)
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_(twins, max_norm)
    fresh.step()
    f, lr, mu, wd32 = float(sc[1].double()), f32(LR), f32(momentum), f32(wd)
    worst = [0.0, 0.0]
    for i, (p, t, g) in enumerate(zip(params, twins, g3)):
        m_f = opt.state[p].get("momentum_buffer")
        m_t = fresh.state[t].get("momentum_buffer")
        check_update(p_old[i], m_old[i], g, p, m_f, f, LR, momentum, wd)
        r_m, r_p = check_update(p_old[i], m_old[i], g, t, m_t, f, LR, momentum, wd)
        worst = [max(worst[0], r_m), max(worst[1], r_p)]
        po, g64 = p_old[i].double().cpu(), g.double().cpu()
        mo = torch.zeros_like(po) if m_old[i] is None else m_old[i].double().cpu()
        d = f * g64 + wd32 * po
        m64 = mu * mo + d
        p64 = po - lr * m64
        gap_p = (t.detach().double().cpu() - p.detach().double().cpu()).abs()
        assert bool((gap_p <= 8 * EPS * (p64.abs() + lr * m64.abs())).all()), i
        if momentum != 0:
            gap_m = (m_t.double().cpu() - m_f.double().cpu()).abs()
            assert bool((gap_m <= 8 * EPS * (mu * mo.abs() + d.abs())).all()), i
    print(f"\n[torch twin] case {(momentum, wd, max_norm)}: torch's third step, worst m err / bound {worst[0]:.3f}, "
          f"worst p err / bound {worst[1]:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 8. repeatable bits
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_bit_repeatable(base):
    momentum, wd, max_norm = CASES[0]
    runs = []
    for _ in range(2):
        ps, ms = place(base["p"], (OFF_ALL,)), place(base["m"], (OFF_ALL,))
        scs = [run_entries(ps, place(base["g"][s], (OFF_ALL, OFF_G)), ms, LR, momentum, wd, max_norm).clone() for s in range(2)]
        runs.append((ps, ms, scs))
    (p0, m0, s0), (p1, m1, s1) = runs
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert all(torch.equal(a, b) for a, b in zip(m0, m1))
    assert all(torch.equal(a, b) for a, b in zip(s0, s1))


def test_sumsq_bits_do_not_depend_on_alignment(base):
    """The partial sums of a tensor are a function of its length: the same values behind an aligned and an unaligned
    pointer give the same bits."""
    import dgv2_native as N

    idx = [5, 6, 7, 8, 9]
    arrs = [base["g"][0][i] for i in idx]
    out = []
    for off in ((), tuple(range(len(idx)))):
        gs = place(arrs, off)
        parts = torch.zeros((len(gs), N.SUMSQ_PARTS), device=DEV)
        N.call("dgv2_sumsq_list", N.ptr_array(gs), N.int_array([g.numel() for g in gs]), len(gs), N.ptr(parts), N.stream())
        out.append(parts)
    assert torch.equal(out[0], out[1])
    want = torch.tensor([float((torch.from_numpy(a).double() ** 2).sum()) for a in arrs], dtype=torch.float64)
    got = out[0].double().sum(1).cpu()
    assert bool(((got - want).abs() <= 2.0 ** -18 * want).all())


# ---------------------------------------------------------------------------------------------------------------------
# 9. the loss scale
# ---------------------------------------------------------------------------------------------------------------------
def _sgd_with_state(base, momentum=0.9, wd=1e-4):
    params = [torch.nn.Parameter(t) for t in place(base["p"], (OFF_ALL,))]
    opt = torch.optim.SGD(params, lr=LR, momentum=momentum, weight_decay=wd)
    for p, m in zip(params, place(base["m"], (OFF_ALL,))):
        opt.state[p]["momentum_buffer"] = m
    return params, opt


def test_overflow_skips_the_step_and_backs_off(base):
    from gans.models.ops.native import fused_clip_sgd_step

    params, opt = _sgd_with_state(base)
    for p, g in zip(params, place(base["g"][0])):
        p.grad = g
    params[9].grad[12345] = float("inf")
    p_old, m_old = snapshot(params), snapshot([opt.state[p]["momentum_buffer"] for p in params])
    state = torch.tensor([1024.0, 0.0], device=DEV)
    sc = fused_clip_sgd_step(opt, 1.0, scale_state=state)
    assert float(sc[2]) == 1 and float(sc[3]) == 1024
    assert state.tolist() == [512.0, 0.0]
    for i, p in enumerate(params):
        assert torch.equal(p.detach(), p_old[i]) and torch.equal(opt.state[p]["momentum_buffer"], m_old[i]), i
    # without a loss scale the same gradient goes on into the parameters, as in the reference
    sc = fused_clip_sgd_step(opt, 1.0)
    assert float(sc[2]) == 0 and not bool(torch.isfinite(params[9].detach()).all())


def test_growth_and_scaled_gradients(base):
    from gans.models.ops.native import fused_clip_sgd_step

    scaled, opt_s = _sgd_with_state(base)
    plain, opt_p = _sgd_with_state(base)
    state = torch.tensor([1024.0, 0.0], device=DEV)
    want_state = [[1024.0, 1.0], [2048.0, 0.0]]
    for s in range(2):
        for a, b, g in zip(scaled, plain, place(base["g"][s])):
            a.grad = g * 1024.0         # what backward of loss * 1024 leaves
            b.grad = g.clone()
        sc_s = fused_clip_sgd_step(opt_s, 1.0, scale_state=state, growth_interval=2).clone()
        sc_p = fused_clip_sgd_step(opt_p, 1.0).clone()
        assert state.tolist() == want_state[s]
        assert float(sc_s[2]) == 0 and float(sc_s[3]) == 1024
        assert abs(float(sc_s[0]) - float(sc_p[0])) <= 2.0 ** -18 * float(sc_p[0])
    lr = f32(LR)
    for a, b in zip(scaled, plain):
        pa, pb = a.detach().double().cpu(), b.detach().double().cpu()
        mb = opt_p.state[b]["momentum_buffer"].double().cpu()
        assert bool(((pa - pb).abs() <= 8 * EPS * (pb.abs() + lr * mb.abs())).all())


# ---------------------------------------------------------------------------------------------------------------------
# 10 - 13. the Trainer
# ---------------------------------------------------------------------------------------------------------------------
B, H, W = 2, 3, 48


def tiny_cfg(use_amp=False, lr_decay_steps=10000):
    from semseg.config import load_config

    cfg = load_config(os.path.join(GOLDEN, "semseg_cfg", "sim2real_w_gan_noise_dustyv2.yaml"))    # 3 classes, xyz + depth, CRF
    cfg.dataset.shape = [H, W]
    cfg.training.batch_size = B
    cfg.training.lr_decay_steps = lr_decay_steps
    cfg.use_amp = use_amp
    assert cfg.arch.inputs == ["xyz", "depth"] and cfg.arch.use_crf and cfg.dataset.num_classes == 3
    return cfg


def batches(n, seed=0):
    from semseg.datasets import SyntheticFrontal

    ds = SyntheticFrontal(n * B, (H, W), 3, seed=seed)
    loader = torch.utils.data.DataLoader(ds, batch_size=B)
    return [{k: v.to(DEV) for k, v in item.items()} for item in loader]


def make_trainer(**kw):
    from semseg.trainer import Trainer

    torch.manual_seed(0)
    return Trainer(tiny_cfg(**{k: v for k, v in kw.items() if k in ("use_amp", "lr_decay_steps")}), DEV,
                   fused_optimizer=kw.get("fused_optimizer", True), pretrained_weights=False)


def checked_step(trainer, item):
    """trainer.step(item) with the optimizer's output held to the float64 update from the gradient the step left.
    Only step() itself runs under the caller's sync-debug mode; the readbacks of the check run with it lifted.
    -> (step output, norm error, worst element error / bound)"""
    params = list(trainer.model.parameters())
    group = trainer.optimizer.param_groups[0]
    lr = group["lr"]
    p_old = snapshot(params)
    m_old = snapshot([trainer.optimizer.state[p].get("momentum_buffer") for p in params])
    out = trainer.step(item)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("default")
    try:
        sc = trainer.optimizer._dgv2_sc
        assert all(p.grad is not None for p in params)
        e_norm, _ = check_scalars(sc, [p.grad for p in params], trainer.max_grad_norm)
        assert float(out["grad_norm"]) == float(sc[0])
        f = float(sc[1].double())
        worst = 0.0
        for i, p in enumerate(params):
            worst = max(worst, *check_update(p_old[i], m_old[i], p.grad, p, trainer.optimizer.state[p]["momentum_buffer"], f,
                                             lr, group["momentum"], group["weight_decay"]))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    return out, e_norm, worst


def test_trainer_step_fp32():
    trainer = make_trainer()
    items = batches(3)
    assert len(list(trainer.model.parameters())) > 72
    out, e_norm, worst = checked_step(trainer, items[0])
    print(f"\n[trainer fp32] step 1: norm rel err {e_norm:.3e}, worst element err / bound {worst:.3f}")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")     # steps 2 and 3: any host synchronisation inside step() raises
    try:
        for item in items[1:]:
            out, e_norm, worst = checked_step(trainer, item)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"[trainer fp32] step 3: norm rel err {e_norm:.3e}, worst element err / bound {worst:.3f}")
    assert out["loss"].ndim == 0 and bool(torch.isfinite(out["loss"]))
    assert out["pred"].shape == (B, H, W) and out["pred"].dtype == torch.int64
    assert int(trainer.conf_train.sum()) == 3 * B * H * W
    assert trainer.step_count == 3


def test_trainer_unfused_path_agrees():
    """Torch's clip_grad_norm_ + SGD.step from the same initial state: within 1e-5 max|p| after one step (loose on
    purpose: the two backward passes are separate runs of the library's conv backward)."""
    fused = make_trainer()
    plain = make_trainer(fused_optimizer=False)
    plain.model.load_state_dict(fused.model.state_dict())
    (item,) = batches(1)
    outs = []
    for tr in (fused, plain):
        torch.manual_seed(11)      # the head's dropout draws
        outs.append(tr.step(item))
    scale = max(float(p.detach().abs().max()) for p in fused.model.parameters())
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(fused.model.parameters(), plain.model.parameters()))
    moved = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(fused.model.parameters(), make_trainer().model.parameters()))
    print(f"\n[trainer] fused vs torch tail after one step: max |dp| {diff:.3e} = {diff / scale:.3e} max|p| (step moved {moved:.3e})")
    assert moved > 0
    assert diff <= 1e-5 * scale
    assert abs(float(outs[0]["loss"]) - float(outs[1]["loss"])) <= 1e-5 * abs(float(outs[1]["loss"]))
    assert abs(float(outs[0]["grad_norm"]) - float(outs[1]["grad_norm"])) <= 1e-4 * float(outs[1]["grad_norm"])


def test_trainer_step_amp():
    trainer = make_trainer(use_amp=True)
    before = snapshot(list(trainer.model.parameters()))
    for item in batches(3):
        out = trainer.step(item)
        assert bool(torch.isfinite(out["loss"]))
    scale, tracker = trainer.scale.tolist()
    halvings = np.log2(65536.0 / scale)
    assert halvings == int(halvings) and 0 <= halvings <= 3
    assert tracker <= 3
    changed = any(not torch.equal(a, b.detach()) for a, b in zip(before, trainer.model.parameters()))
    assert changed or halvings > 0
    assert trainer.loss_scale() == scale
    print(f"\n[trainer amp] loss scale after three steps {scale:g}, tracker {tracker:g}, parameters changed: {changed}")


def test_validate_matches_evaluator_by_hand():
    from semseg.metrics import Evaluator
    from semseg.trainer import make_inputs

    trainer = make_trainer()
    items = batches(2, seed=3)
    got = trainer.validate(items)
    assert trainer.model.training
    ev = Evaluator(3)
    trainer.model.eval()
    with torch.inference_mode():
        for item in items:
            logit = trainer.model(make_inputs(item, ["xyz", "depth"]), item["xyz"], item["mask"])
            ev.update(logit, item["label"], item["mask"])
    want = ev.summary(mean_classes=slice(1, 3))
    for key in ("tp", "fp", "fn"):
        np.testing.assert_array_equal(got[key], want[key])
    assert int(ev.conf.sum()) == 2 * B * H * W
    np.testing.assert_allclose(got["iou"], want["iou"], rtol=0, atol=0)


def test_checkpoint_round_trip():
    from gans.models.ops.native import fused_clip_sgd_step

    a = make_trainer(lr_decay_steps=2)
    items = batches(3)
    for item in items[:2]:
        a.step(item)
    blob = io.BytesIO()
    torch.save(a.state_dict(), blob)
    blob.seek(0)
    ckpt = torch.load(blob, map_location="cpu", weights_only=True)      # plain containers only: cfg is a dict
    assert set(ckpt) == {"cfg", "step", "model", "optim", "scale"} and type(ckpt["cfg"]) is dict and ckpt["step"] == 2
    b = make_trainer(lr_decay_steps=2)
    b.load_state_dict(ckpt)
    legacy = {k: v for k, v in ckpt.items() if k != "scale"}
    make_trainer(lr_decay_steps=2, use_amp=True).load_state_dict(legacy)      # a checkpoint without "scale" still loads
    lr = a.optimizer.param_groups[0]["lr"]
    assert lr == 0.05 * 0.5 and b.optimizer.param_groups[0]["lr"] == lr and b.step_count == 2
    pa, pb = list(a.model.parameters()), list(b.model.parameters())
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach(), y.detach())
        assert torch.equal(a.optimizer.state[x]["momentum_buffer"], b.optimizer.state[y]["momentum_buffer"])
    for (ka, x), (kb, y) in zip(a.model.state_dict().items(), b.model.state_dict().items()):
        assert ka == kb and torch.equal(x, y), ka
    # the same gradient through both optimizers: the same bits
    for i, (x, y) in enumerate(zip(pa, pb)):
        g = torch.from_numpy(hash_unit(9, i, x.numel()) * np.float32(0.01)).to(DEV).reshape(x.shape)
        x.grad, y.grad = g, g.clone()
    sa = fused_clip_sgd_step(a.optimizer, a.max_grad_norm).clone()
    sb = fused_clip_sgd_step(b.optimizer, b.max_grad_norm).clone()
    assert torch.equal(sa, sb)
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach(), y.detach())
        assert torch.equal(a.optimizer.state[x]["momentum_buffer"], b.optimizer.state[y]["momentum_buffer"])
    # and the loaded trainer's next step holds the float64 check; its schedule goes on from the checkpoint
    checked_step(b, items[2])
    assert b.step_count == 3 and b.optimizer.param_groups[0]["lr"] == lr
    b.step(items[0])
    assert b.optimizer.param_groups[0]["lr"] == lr * 0.5


class TwoScaleStub(torch.nn.Module):
    """Logits at half width and at full size, as a deeply supervised model returns them in training."""

    def __init__(self, in_ch, num_classes):
        super().__init__()
        self.coarse = torch.nn.Conv2d(in_ch, num_classes, 3, (1, 2), 1)
        self.fine = torch.nn.Conv2d(in_ch, num_classes, 3, 1, 1)

    def forward(self, img, xyz=None, mask=None):
        return self.coarse(img), self.fine(img)


def test_trainer_step_with_a_tuple_of_logits(monkeypatch):
    """The deep-supervision branch: one masked loss per scale on nearest-exact resized label and mask, summed; the
    predictions and the confusion counts come from the last scale alone."""
    import semseg.trainer as ST

    monkeypatch.setattr(ST, "build_model", lambda cfg, pretrained_weights=True: TwoScaleStub(4, 3))
    trainer = make_trainer()
    assert isinstance(trainer.model, TwoScaleStub)
    (item,) = batches(1, seed=7)
    with torch.no_grad():
        coarse, fine = trainer.model(ST.make_inputs(item, ["xyz", "depth"]))
        assert coarse.shape == (B, 3, H, W // 2) and fine.shape == (B, 3, H, W)
        label_c = torch.nn.functional.interpolate(item["label"][:, None].float(), size=(H, W // 2), mode="nearest-exact")[:, 0].long()
        mask_c = torch.nn.functional.interpolate(item["mask"][:, None], size=(H, W // 2), mode="nearest-exact")[:, 0]
        assert torch.equal(label_c, item["label"][:, :, 1::2]) and torch.equal(mask_c, item["mask"][:, :, 1::2])
        loss_c, _ = trainer.criterion(coarse, label_c, mask_c)
        loss_f, pred_f = trainer.criterion(fine, item["label"], item["mask"])
        want = (loss_c + loss_f) * trainer.loss_coef
    out, _, worst = checked_step(trainer, item)
    assert abs(float(out["loss"]) - float(want)) <= 4 * EPS * abs(float(want))
    assert torch.equal(out["pred"], pred_f) and out["pred"].shape == (B, H, W)
    assert int(trainer.conf_train.sum()) == B * H * W          # the last scale only
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in trainer.model.parameters())
    assert worst <= 1


def test_fused_step_skips_empty_parameters(base):
    from gans.models.ops.native import fused_clip_sgd_step

    params = [torch.nn.Parameter(t) for t in place(base["p"][:4])] + [torch.nn.Parameter(torch.zeros(0, device=DEV))]
    opt = torch.optim.SGD(params, lr=LR, momentum=0.9)
    for p, g in zip(params, place(base["g"][0][:4]) + [torch.zeros(0, device=DEV)]):
        p.grad = g
    p_old = snapshot(params)
    sc = fused_clip_sgd_step(opt, 0.0)
    assert sc is opt._dgv2_sc                                    # one buffer, overwritten by the next step
    for i in range(4):
        check_update(p_old[i], None, params[i].grad, params[i], opt.state[params[i]]["momentum_buffer"], float(sc[1]), LR, 0.9, 0.0)
    assert "momentum_buffer" not in opt.state[params[4]]


# ---------------------------------------------------------------------------------------------------------------------
# 14. the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_synthetic_run(tmp_path):
    import yaml

    from semseg.config import to_plain

    cfg = tiny_cfg(use_amp=True)
    cfg.training.checkpoint.stats = 2
    cfg.training.checkpoint.test = 4
    cfg_path = tmp_path / "tiny.yaml"
    cfg_path.write_text(yaml.safe_dump(to_plain(cfg)))
    out_dir = tmp_path / "run"
    cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.join(ROOT, "train_semseg.py"), "--config", str(cfg_path),
           "--synthetic", "--max_steps", "4", "--batch_size", str(B), "--out_dir", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    def strict(token):
        raise AssertionError(f"{token} in the log: not JSON")

    rows = [json.loads(line, parse_constant=strict) for line in (out_dir / "train_log.jsonl").read_text().splitlines()]
    train_rows = [row for row in rows if "loss" in row]
    assert [row["step"] for row in train_rows] == [2, 4]
    for row in train_rows:
        assert {"step", "loss", "lr", "grad_norm", "skipped_steps", "loss_scale", "iou"} <= set(row)
        assert len(row["iou"]) == 3 and row["lr"] == 0.05 and np.isfinite(row["loss"])
        assert row["grad_norm"] is None or np.isfinite(row["grad_norm"])
        assert 0 <= row["skipped_steps"] <= 2 and (row["grad_norm"] is not None or row["skipped_steps"] == 2)
    val_rows = [row for row in rows if "val_iou" in row]
    assert [row["step"] for row in val_rows] == [4] and len(val_rows[0]["val_iou"]) == 3
    ckpts = sorted((out_dir / "models").glob("*.pth"))
    assert [c.name for c in ckpts] == ["checkpoint_step-0000000004.pth"]
    ckpt = torch.load(ckpts[0], map_location="cpu", weights_only=True)
    assert ckpt["step"] == 4 and ckpt["cfg"]["dataset"]["shape"] == [H, W] and ckpt["scale"] is not None
    tr = make_trainer(use_amp=True)
    tr.load_state_dict(ckpt)
    assert tr.step_count == 4 and float(tr.scale[0]) == ckpt["scale"][0]
