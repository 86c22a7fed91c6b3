"""The ORDER of one training iteration, mode by mode, against tests/golden/step_order.json: which bodies run, where the
reals are fetched, where each gradient reduction starts and is joined, where Adam, the EMA update and the tail exchange
stand (events of tests/step_recorder.py).  The fixture was recorded from the 170-line Trainer.step that preceded the
sub-step layout and is what that layout, and any later one, has to reproduce.

Small configuration (16x64, B = 8 per rank, lazy.gp = 2: R1 is due on iterations 2 and 4), every draw injected.
In-process modes run eagerly for 4 iterations; the child-process modes go through tests/dist_child.py.

    python tests/test_gpu_step_order.py --record [mode ...]      rewrites the fixture's entries (all modes by default)
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "step_order.json")

# mode -> (environment, cfg.training overrides, chunks per iteration)
IN_PROCESS = {
    "plain": ({}, {}, 1),
    "no_fused_opt": ({"DGV2_NO_FUSED_OPT": "1"}, {}, 1),
    "overlap_d_reduce": ({}, {"overlap_d_reduce": True}, 1),
    "accumulate2": ({}, {}, 2),
    "ragan": ({}, {"gan_objective": "ragan"}, 1),
    "path_length": ({}, {}, 1),
}
# mode -> (world, iterations, hip_graph, environment)
CHILDREN = {
    "rccl1_eager": (1, 4, False, {"DGV2_DIST_WORLD1": "1"}),
    "rccl1_graph_folded": (1, 8, True, {"DGV2_DIST_WORLD1": "1"}),
    "rccl1_graph_side_stream": (1, 8, True, {"DGV2_DIST_WORLD1": "1", "DGV2_NO_FOLDED_REDUCE": "1"}),
    "gloo2_eager": (2, 4, False, {}),
}


def _in_process(mode, monkeypatch):
    import dist_child
    import step_recorder
    from gans.trainer import Trainer
    from helpers import small_cfg
    env, training, nacc = IN_PROCESS[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = small_cfg()
    cfg.dataset.name = "synthetic"
    cfg.training.update(rank=0, num_gpus=1, batch_size=8, batch_size_per_gpu=8, resume=None, hip_graph=False, **training)
    cfg.training.lazy.update(gp=2, ada=2)
    cfg.training.augment.update(p_init=0.5, kimg=1)
    cfg.training.warmup.fade_kimg = 0
    if mode == "path_length":     # the configuration of tests/test_gpu_pl.py::test_trainer_runs_the_regulariser, R1 every 2nd
        cfg.training.loss.pl = 2.0
        cfg.training.lazy.update(gp=2, pl=2, ada=4)
    torch.manual_seed(0)
    tr = Trainer(cfg, sync_scalars=False)
    if nacc > 1:
        tr.batch_size, tr.num_accumulation = 8 * nacc, nacc     # what Trainer.__init__ derives from batch_size = 16
    rec = step_recorder.install()
    try:
        trace = []
        for it in range(1, 5):
            d, depth, mask = dist_child.draws_for(it, 1)
            if mode == "path_length":
                g = torch.Generator().manual_seed(3000 + it)
                d["pl.shifts"] = torch.rand(8, generator=g) * 6.2831853
                d["pl.u"] = torch.rand(8, 1, 16, 64, generator=g).clamp(1e-6, 1 - 1e-6)
            tr.set_draws(d)
            tr.iter_train_loader = iter([{"depth": depth.cuda(), "mask": mask.cuda()}] * nacc)
            rec.take()
            out = tr.step(it)
            trace.append(rec.take())
            assert all(torch.isfinite(v).all() for v in out.values() if torch.is_tensor(v)), (mode, it)
    finally:
        rec.uninstall()
    return trace


def _children(mode, out_dir):
    """The ranks' traces.  Each child runs under a time limit of its own; a child that fails or runs out of time ends
    the mode (the others are killed, nothing further is started)."""
    from test_gpu_dist import _free_port
    world, iters, graph, extra = CHILDREN[mode]
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", DGV2_TEST_STEP_TRACE="1", **extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_child.py"), str(out_dir), str(world), str(r), port,
                               str(iters), str(int(graph))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    try:
        logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    return [torch.load(os.path.join(out_dir, f"rank{r}_of{world}.pt"), weights_only=False)["trace"] for r in range(world)]


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _assert_same(mode, got, want):
    assert len(got) == len(want), (mode, len(got), len(want))
    for it, (a, b) in enumerate(zip(got, want), 1):
        assert a == b, (mode, "iteration", it, "got", a, "want", b)


@pytest.mark.parametrize("mode", list(IN_PROCESS))
def test_in_process_step_order(mode, monkeypatch):
    _assert_same(mode, _in_process(mode, monkeypatch), _fixture()[mode])


@pytest.mark.parametrize("mode", list(CHILDREN))
def test_child_process_step_order(mode, tmp_path):
    ranks = _children(mode, tmp_path)
    for r, trace in enumerate(ranks):     # every rank of a run issues the same sequence (one communicator, one order)
        _assert_same((mode, "rank", r), json.loads(json.dumps(trace)), _fixture()[mode])


if __name__ == "__main__":
    import tempfile
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "dusty-gan-v2_amd"), os.path.join(HERE, "golden")]
    assert sys.argv[1] == "--record", __doc__
    modes = sys.argv[2:] or list(IN_PROCESS) + list(CHILDREN)
    fixture = _fixture() if os.path.exists(FIXTURE) else {}
    for mode in modes:
        if mode in IN_PROCESS:
            with pytest.MonkeyPatch.context() as mp:
                fixture[mode] = _in_process(mode, mp)
        else:
            with tempfile.TemporaryDirectory() as t:
                ranks = _children(mode, t)
            assert all(r == ranks[0] for r in ranks), mode
            fixture[mode] = ranks[0]
        with open(FIXTURE, "w") as f:     # after every mode: a mode that fails leaves the earlier ones recorded
            f.write("{\n" + ",\n".join(f' "{m}": [\n' + ",\n".join("  " + json.dumps(it) for it in tr) + "\n ]"
                                       for m, tr in fixture.items()) + "\n}\n")
        print("recorded", mode, [len(it) for it in fixture[mode]], flush=True)
