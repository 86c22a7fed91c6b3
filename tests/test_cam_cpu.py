"""CPU checks of the segmentation evaluation path: the context-aggregation fixture and its restatement, the native
wrapper's range table and refusals, the routing rule, the checkpoint loader of semseg.pretrained (both layouts) and the
argument parser of the command line test_semseg.py.  Nothing here launches a kernel.

The reference-layout checkpoint is built on the class-stub path that tests/test_checkpoint_compat.py's fixture uses:
omegaconf is not importable where the fixtures are made, so classes with omegaconf's module paths, names and attribute
layout (DictConfig / ListConfig._content, value nodes ._val) are pickled; the loader under test never imports them."""
import ctypes
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

import cam_ref as R
from conftest import GOLDEN, ROOT
from test_abi import HEADER, parse_header


@pytest.fixture(scope="module")
def fx():
    d = np.load(os.path.join(GOLDEN, "cam.npz"))
    return {k: d[k] for k in d.files}


def _make_cam(i):
    from semseg.models.squeezeseg_v2 import CAM
    B, C, H, W, kind = R.CAM_CASES[i]
    cam = CAM(C, R.REDUCTION)
    sd = R.cam_case_state_dict(i, cam.state_dict())
    cam.load_state_dict(sd, strict=True)
    return cam.eval(), sd


# ---- fixture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.CAM_CASES)))
def test_fixture_is_self_consistent(fx, i):
    """The restatement reproduces the stored float64 output of the reference's module, this project's module on the
    CPU reproduces its float32 output within E_ref, and the stored error figures describe the stored sample."""
    name = R.cam_case_name(i)
    B, C, H, W, kind = R.CAM_CASES[i]
    cam, sd = _make_cam(i)
    assert list(sd) == ["attn.1.weight", "attn.1.bias", "attn.3.weight", "attn.3.bias"]
    assert tuple(sd["attn.1.weight"].shape) == (C // 16, C, 1, 1) and tuple(sd["attn.3.weight"].shape) == (C, C // 16, 1, 1)
    x = R.cam_case_input(i)
    idx = R.sample_index(name, x.numel())
    ref64 = R.cam_ref(sd, x)
    top, e_ref = float(fx[name + "/max64"]), float(fx[name + "/e_ref"])
    assert abs(float(ref64.abs().max()) - top) <= 1e-12 * top
    assert float((ref64.flatten()[idx] - torch.from_numpy(fx[name + "/ref64"])).abs().max()) <= 1e-12 * top
    with torch.no_grad():
        mine32 = cam(x.clone())
    assert float((mine32.double() - ref64).abs().max()) <= 2.0 * e_ref + 2.0 ** -22 * top
    sample_err = float((torch.from_numpy(fx[name + "/ref32"]).double() - torch.from_numpy(fx[name + "/ref64"])).abs().max())
    assert 0 < sample_err <= e_ref
    assert 0 < float(fx[name + "/e_ref_border"]) <= e_ref and float(fx[name + "/max64_border"]) <= top
    if kind == "negative":
        assert float(x.max()) < -0.9 and bool(R.border_mask(H, W).any())
    if kind == "corners":
        corners = torch.tensor([0, W - 1, (H - 1) * W, H * W - 1])
        assert bool(torch.isin(x.flatten(2).argmax(dim=2), corners).all())


def test_restatement_pads_with_minus_infinity():
    """x = -2 everywhere on 2 x 2, w1 = -1/16, w2 = 1, no biases: the pooled maximum is -2, so a = 2 and the gate is
    sigmoid(2); a zero-padded maximum would be 0 in every pixel, a = 0 and the gate 1/2."""
    sd = {"attn.1.weight": torch.full((1, 16, 1, 1), -1.0 / 16), "attn.1.bias": torch.zeros(1),
          "attn.3.weight": torch.ones(16, 1, 1, 1), "attn.3.bias": torch.zeros(16)}
    y = R.cam_ref(sd, torch.full((1, 16, 2, 2), -2.0))
    want = -2.0 / (1.0 + np.exp(-2.0))
    assert float((y - want).abs().max()) <= 1e-15 and abs(want - (-1.0)) > 0.7


# ---- the wrapper ----------------------------------------------------------------------------------------------------
def test_cam_supported_table():
    from gans.models.ops import native
    from gans.models.ops.native import cam as M
    assert native.cam_forward is M.cam_forward and native.cam_supported is M.cam_supported
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for C in (16, 32, 48, 64, 96, 112, 128):
            assert M.cam_supported(C, C // 16, dtype), (C, dtype)
        for Cr in range(1, 9):
            assert M.cam_supported(128, Cr, dtype)
    for C, Cr in ((0, 1), (8, 1), (24, 1), (144, 9), (144, 8), (256, 16), (64, 0), (64, 9), (64.0, 4), (64, 4.0)):
        assert not M.cam_supported(C, Cr, torch.float32), (C, Cr)
    for dtype in (torch.float64, torch.int32, torch.int8):
        assert not M.cam_supported(64, 4, dtype)
    assert (M.CAM_C_MAX, M.CAM_CR_MAX, M.CAM_SAMPLE_MAX) == (128, 8, 2 ** 31 - 1)


def test_entry_declared_bound_and_abi_unchanged():
    import dgv2_native as N
    protos = parse_header()
    assert protos["dgv2_cam_fwd"] == ["ptr"] * 6 + ["int"] * 6 + ["ptr"]
    assert N.SIGNATURES["dgv2_cam_fwd"] == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert N.ABI_VERSION == 60 and N.lib.dgv2_abi_version() == 60
    src = open(HEADER).read()
    for needle in ("squeezeseg_v2.py:20-36", "the padding is -inf, not 0", "fmaf(w1[j][c], m[c], t_c)",
                   "fmaf(w2[c][j], a[j], u_j)", "1 / (1 + expf(-s[c]))"):
        assert needle in src, needle


def test_entry_refuses_bad_arguments_before_launching():
    """Every refusal is DGV2_EINVAL before anything is launched: the pointers are never dereferenced."""
    import dgv2_native as N
    fake = 0x1000
    good = dict(y=fake, x=fake, w1=fake, b1=fake, w2=fake, b2=fake, B=1, C=64, Cr=4, H=8, W=8, dtype=N.F32)

    def call(**over):
        a = dict(good, **over)
        return N.lib.dgv2_cam_fwd(a["y"], a["x"], a["w1"], a["b1"], a["w2"], a["b2"], a["B"], a["C"], a["Cr"], a["H"],
                                  a["W"], a["dtype"], None)

    bad = [dict(y=None), dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(B=0), dict(H=0),
           dict(W=-1), dict(C=0), dict(C=8), dict(C=24), dict(C=144), dict(Cr=0), dict(Cr=9), dict(dtype=2), dict(dtype=7),
           dict(C=128, H=4096, W=4096),            # 2^31 elements in a sample: one past the 32-bit offsets
           dict(C=16, H=65536, W=2048)]
    for over in bad:
        assert call(**over) == N.EINVAL, over


def test_wrapper_refuses_before_the_library():
    from gans.models.ops.native import cam as M
    w1, b1, w2, b2 = torch.zeros(4, 64, 1, 1), torch.zeros(4), torch.zeros(64, 4, 1, 1), torch.zeros(64)
    x = torch.zeros(1, 64, 4, 4)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):        # CPU tensors: no fallback
        M.cam_forward(x, w1, b1, w2, b2)
    with pytest.raises(ValueError, match="outside the kernel's range"):
        M.cam_forward(torch.zeros(1, 24, 4, 4), torch.zeros(1, 24, 1, 1), torch.zeros(1), torch.zeros(24, 1, 1, 1), torch.zeros(24))
    with pytest.raises(ValueError, match="outside the kernel's range"):
        M.cam_forward(x.double(), w1, b1, w2, b2)
    with pytest.raises(ValueError, match="w2 must have shape"):
        M.cam_forward(x, w1, b1, torch.zeros(64, 2, 1, 1), b2)
    with pytest.raises(ValueError, match="b1 must have shape"):
        M.cam_forward(x, w1, None, w2, b2)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        M.cam_forward(x[0], w1, b1, w2, b2)
    with pytest.raises(ValueError, match="empty input"):
        M.cam_forward(torch.zeros(0, 64, 4, 4), w1, b1, w2, b2)
    # a sample of 2^31 elements: refused from the shape alone (an expanded view: no memory behind it)
    huge = torch.zeros(1, 1, 1, 1).expand(1, 64, 8192, 4096)
    with pytest.raises(ValueError, match="32-bit offsets"):
        M.cam_forward(huge, w1, b1, w2, b2)


# ---- routing --------------------------------------------------------------------------------------------------------
def test_routing_rule_is_false_off_the_native_path(monkeypatch):
    from semseg.models import common
    cam, _ = _make_cam(1)
    x = R.cam_case_input(1)
    assert common.CAM_NATIVE in (True, False)

    class OnDevice:
        """what the rule reads of a tensor, claiming to be on the GPU"""
        is_cuda, ndim, dtype = True, 4, torch.float32

    monkeypatch.setattr(common, "CAM_NATIVE", True)
    with torch.no_grad():
        assert not common.cam_uses_native(cam, x)               # a CPU tensor
        assert common.cam_uses_native(cam, OnDevice())          # the same module on a CUDA input
        OnDevice.dtype = torch.float64
        assert not common.cam_uses_native(cam, OnDevice())
        OnDevice.dtype = torch.float16
        assert common.cam_uses_native(cam, OnDevice())
        monkeypatch.setattr(common, "CAM_NATIVE", False)        # read at every call
        assert not common.cam_uses_native(cam, OnDevice())
        monkeypatch.setattr(common, "CAM_NATIVE", True)
        cam.train()
        assert not common.cam_uses_native(cam, OnDevice())      # train()
        cam.eval()
    assert torch.is_grad_enabled() and not common.cam_uses_native(cam, OnDevice())   # grad mode on
    with torch.inference_mode():
        assert common.cam_uses_native(cam, OnDevice())
    # off the native path the module is the composition: the reference's float32 arithmetic on the CPU
    with torch.no_grad():
        assert torch.equal(cam(x), x * cam.attn(x))
    y = cam(x.clone().requires_grad_(True))
    assert y.requires_grad


# ---- checkpoints ----------------------------------------------------------------------------------------------------
def _small_cfg(use_crf=True):
    from semseg.config import default_config
    cfg = default_config()
    cfg.dataset.shape = [8, 64]
    cfg.arch.use_crf = use_crf
    return cfg


def test_load_checkpoint_round_trips_a_trainer_state_dict(tmp_path):
    from gans.config import Config
    from semseg.pretrained import build_from_checkpoint, load_checkpoint
    from semseg.trainer import Trainer
    torch.manual_seed(3)
    trainer = Trainer(_small_cfg(), "cpu", pretrained_weights=False)
    path = tmp_path / "ckpt.pth"
    torch.save(trainer.state_dict(), path)
    ckpt = load_checkpoint(path)
    assert set(ckpt) == {"cfg", "step", "model", "optim", "scale"} and ckpt["step"] == 0
    cfg = ckpt["cfg"]
    assert isinstance(cfg, Config) and isinstance(cfg.arch.crf, Config)
    assert cfg.arch.name == "squeezeseg_v2" and cfg.dataset.shape == [8, 64] and cfg.arch.crf.theta_beta[2] == 0.01
    model = build_from_checkpoint(ckpt, "cpu")
    assert not model.training and model.crf is not None
    want = trainer.model.state_dict()
    got = model.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        load_checkpoint(tmp_path / "absent.pth")
    torch.save({"G": {}}, tmp_path / "other.pth")
    with pytest.raises(ValueError, match="not a segmentation checkpoint"):
        load_checkpoint(tmp_path / "other.pth")
    # strict=True: a missing key is an error, not a partly loaded model
    broken = dict(ckpt, model={k: v for k, v in ckpt["model"].items() if k != "decoder.head.1.bias"})
    with pytest.raises(RuntimeError, match="decoder.head.1.bias"):
        build_from_checkpoint(broken, "cpu")


def _stub_omegaconf_tree(obj, monkeypatch):
    """`obj` (plain containers) as a tree of classes with omegaconf's module paths, names and attribute layout."""
    mods = {}
    for name in ("omegaconf", "omegaconf.base", "omegaconf.dictconfig", "omegaconf.listconfig", "omegaconf.nodes"):
        m = types.ModuleType(name)
        m.__path__ = []
        monkeypatch.setitem(sys.modules, name, m)
        mods[name] = m

    def cls(module, name, base=object):
        c = type(name, (base,), {"__module__": module})
        setattr(mods[module], name, c)
        return c

    Metadata = cls("omegaconf.base", "Metadata")
    ContainerMetadata = cls("omegaconf.base", "ContainerMetadata", Metadata)
    DictConfig, ListConfig = cls("omegaconf.dictconfig", "DictConfig"), cls("omegaconf.listconfig", "ListConfig")
    nodes = {bool: cls("omegaconf.nodes", "BooleanNode"), int: cls("omegaconf.nodes", "IntegerNode"),
             float: cls("omegaconf.nodes", "FloatNode"), str: cls("omegaconf.nodes", "StringNode"),
             type(None): cls("omegaconf.nodes", "AnyNode")}

    def meta(container, key):
        m = (ContainerMetadata if container else Metadata)()
        m.__dict__.update(ref_type=object, object_type=dict if container else None, optional=True, key=key, flags={},
                          flags_root=False, resolver_cache={})
        return m

    def wrap(v, parent, key):
        if isinstance(v, dict):
            n = DictConfig()
            n.__dict__.update(_metadata=meta(True, key), _parent=parent, _flags_cache=None, _content={})
            for k, item in v.items():
                n._content[k] = wrap(item, n, k)
            return n
        if isinstance(v, (list, tuple)):
            n = ListConfig()
            n.__dict__.update(_metadata=meta(True, key), _parent=parent, _flags_cache=None, _content=[])
            for j, item in enumerate(v):
                n._content.append(wrap(item, n, j))
            return n
        n = nodes.get(type(v), nodes[type(None)])()
        n.__dict__.update(_metadata=meta(False, key), _parent=parent, _val=v)
        return n

    return wrap(obj, None, None)


def test_load_checkpoint_reads_the_reference_layout(tmp_path, monkeypatch):
    """{"cfg": <pickled OmegaConf tree>, "step", "model", "optim"}, with a cfg that LACKS keys the defaults supply."""
    from gans.config import Config
    from semseg.config import to_plain
    from semseg.pretrained import build_from_checkpoint, load_checkpoint
    from semseg.trainer import build_model
    cfg = _small_cfg(use_crf=False)
    cfg.arch.inputs = ["xyz", "depth", "mask"]
    cfg.dataset.num_classes = 3
    cfg.dataset.logit_bias = None
    torch.manual_seed(4)
    model = build_model(cfg, pretrained_weights=False)
    plain = to_plain(cfg)
    del plain["training"], plain["loss"], plain["arch"]["crf"]["theta_beta"]
    path = tmp_path / "reference_layout.pth"
    torch.save({"cfg": _stub_omegaconf_tree(plain, monkeypatch), "step": 50000, "model": model.state_dict(),
                "optim": torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9).state_dict()}, path)
    for name in [n for n in sys.modules if n.split(".")[0] == "omegaconf"]:
        monkeypatch.delitem(sys.modules, name)            # the loader never imports what wrote the file
    ckpt = load_checkpoint(path)
    assert not [n for n in sys.modules if n.split(".")[0] == "omegaconf"]
    got = ckpt["cfg"]
    assert isinstance(got, Config) and type(got.arch) is Config and type(got.arch.inputs) is list
    assert got.arch.inputs == ["xyz", "depth", "mask"] and got.dataset.num_classes == 3 and got.dataset.logit_bias is None
    assert got.arch.use_crf is False and got.arch.bn_momentum == 0.001 and got.dataset.shape == [8, 64]
    assert got.training.lr == 0.05 and got.loss.name == "focal_loss"            # from default_config()
    assert got.arch.crf.theta_beta == [0.015, 0.015, 0.01, 0.01] and got.arch.crf.num_iters == 3
    assert ckpt["step"] == 50000
    loaded = build_from_checkpoint(ckpt, "cpu")
    assert not loaded.training and loaded.crf is None
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in loaded.state_dict().items())


# ---- the command line -----------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("semseg_test_cli", os.path.join(ROOT, "test_semseg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parser_and_report(capsys):
    import json
    cli = _cli()
    ap = cli.build_parser()
    a = ap.parse_args(["--ckpt_path", "m.pth"])
    assert (a.ckpt_path, a.batch_size, a.knn_enabled, a.knn_k, a.knn_kernel_size) == ("m.pth", 32, False, 5, 5)   # the reference's
    assert (a.data_root, a.synthetic, a.shape) == ("data/kitti_raw_frontal", None, None)
    a = ap.parse_args("--ckpt_path m.pth --batch_size 4 --knn_enabled --knn_k 3 --knn_kernel_size 3 --synthetic 4 "
                      "--shape 8 64 --data_root /data/k".split())
    assert (a.batch_size, a.knn_enabled, a.knn_k, a.knn_kernel_size, a.synthetic, a.shape, a.data_root) == \
        (4, True, 3, 3, 4, [8, 64], "/data/k")
    for argv in ([], ["--ckpt_path", "m.pth", "--shape", "8"], ["--ckpt_path", "m.pth", "--synthetic", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    capsys.readouterr()
    summary = {"iou": np.array([0.5, 0.25, float("nan")]), "precision": np.array([1.0, 0.5, 0.0]),
               "recall": np.array([0.5, 1 / 3, 0.0]), "mean_iou": 0.125, "mean_precision": 0.25, "mean_recall": 1 / 6,
               "tp": np.array([2, 1, 0]), "fp": np.array([0, 1, 0]), "fn": np.array([2, 2, 0])}
    lines = cli.format_table(["unknown", "car", "pedestrian"], summary)
    assert lines[0].split() == ["class", "iou", "precision", "recall"] and lines[2].split() == ["car", "25.0%", "50.0%", "33.3%"]
    assert lines[-1].split() == ["mean", "12.5%", "25.0%", "16.7%"] and len(lines) == 5
    rec = json.loads(json.dumps(cli.json_record(a, ["unknown", "car", "pedestrian"], summary, 4), allow_nan=False))
    assert rec["iou"] == [0.5, 0.25, None] and rec["tp"] == [2, 1, 0] and rec["fn"] == [2, 2, 0] and rec["scans"] == 4
    assert rec["mean_iou"] == 0.125 and rec["knn"] is True and rec["classes"] == ["unknown", "car", "pedestrian"]
