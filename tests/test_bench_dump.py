"""bench.py --dump-outputs: what the last timed step computed, as float32 / float64 .npy files of bounded size, with
large arrays sampled at the same positions in every run so that two builds can be compared output for output."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Model(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(n))
        self.register_buffer("stat", torch.ones(3))
        self.register_buffer("count", torch.zeros(2, dtype=torch.long))   # not floating point: not dumped


def _trainer(n_d):
    return types.SimpleNamespace(G=_Model(10), D=_Model(n_d), G_ema=_Model(10), A=types.SimpleNamespace(p=torch.tensor(0.6)))


def test_dump_writes_scalars_and_bounded_state(tmp_path):
    import bench
    torch.manual_seed(0)
    tr = _trainer(bench.DUMP_SAMPLE + 5)
    out = {"loss/G/adversarial": torch.tensor(1.5), "stats/ema_decay": 0.25}
    bench.dump_outputs(str(tmp_path), bench.step_outputs(tr, out))
    files = sorted(os.listdir(tmp_path))
    assert files == ["D.state.npy", "G.state.npy", "G_ema.state.npy", "ada_p.npy",
                     "step.loss_G_adversarial.npy", "step.stats_ema_decay.npy"]
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64)
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "step.loss_G_adversarial.npy").tolist() == [1.5]
    assert np.load(tmp_path / "step.stats_ema_decay.npy").tolist() == [0.25]
    g = np.load(tmp_path / "G.state.npy")
    np.testing.assert_array_equal(g, np.concatenate([tr.G.w.detach().numpy(), np.ones(3, np.float32)]))
    d = np.load(tmp_path / "D.state.npy")
    assert d.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(d, np.concatenate([tr.D.w.detach().numpy(), np.ones(3, np.float32)])).all()


def test_dump_sample_positions_are_fixed(tmp_path):
    import bench
    torch.manual_seed(1)
    tr = _trainer(bench.DUMP_SAMPLE * 2)
    bench.dump_outputs(str(tmp_path / "a"), bench.step_outputs(tr, {}))
    bench.dump_outputs(str(tmp_path / "b"), bench.step_outputs(tr, {}))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "D.state.npy"), np.load(tmp_path / "b" / "D.state.npy"))
