"""CPU tests of the host-side logic that needs no kernel: module surface, state-dict schema, drop-in aliases,
dense helpers vs the oracle, rerank logic, on-disk formats, configuration."""
import os

import numpy as np
import pytest
import torch

from _common import ROOT, filled_state_dict, hash_normalish, manifest_shapes


def _model(B=4):
    from grafp_amd.train import build_model
    from grafp_amd.util import load_config
    cfg = load_config()
    cfg["bsz_train"] = B
    return cfg, build_model(cfg)


def test_state_dict_schema_matches_reference_manifest():
    cfg, model = _model()
    shapes = manifest_shapes()
    sd = model.state_dict()
    assert list(sd.keys()) == list(shapes.keys())                      # same 443 keys, same order
    assert all(tuple(v.shape) == shapes[k] for k, v in sd.items())
    assert sum(p.numel() for p in model.parameters() if p.requires_grad) == 18367264
    assert sum(p.numel() for p in model.parameters() if not p.requires_grad) == 2253312   # frozen relative_pos
    assert len(model.encoder.backbone) == 15 and hasattr(model.encoder, "stem") and hasattr(model.encoder, "proj")
    # a reference-style checkpoint (with or without DataParallel's 'module.' prefix) loads
    from grafp_amd.util import strip_module_prefix
    filled = filled_state_dict()
    full = dict(sd)
    full.update(filled)
    model.load_state_dict(full)
    model.load_state_dict(strip_module_prefix({"module." + k: v for k, v in full.items()}))


def test_constructor_surface():
    import inspect
    from grafp_amd.encoder.graph_encoder import GraphEncoder
    from grafp_amd.modules.transformations import GPUTransformNeuralfp
    from grafp_amd.simclr.simclr import SimCLR
    p = inspect.signature(GraphEncoder.__init__).parameters
    assert [k for k in p][1:] == ["cfg", "k", "conv", "act", "norm", "bias", "dropout", "dilation", "epsilon", "drop_path",
                                  "size", "emb_dims", "in_channels"]
    assert p["k"].default == 3 and p["size"].default == "t" and p["in_channels"].default == 3
    assert [k for k in inspect.signature(SimCLR.__init__).parameters][1:] == ["cfg", "encoder"]
    assert [k for k in inspect.signature(GPUTransformNeuralfp.__init__).parameters][1:] == [
        "cfg", "ir_dir", "noise_dir", "train", "cpu", "abl"]
    from grafp_amd.eval import eval_faiss
    ps = inspect.signature(eval_faiss).parameters
    assert list(ps) == ["emb_dir", "emb_dummy_dir", "index_type", "nogpu", "max_train", "test_ids", "test_seq_len",
                        "k_probe", "n_centroids"]
    assert ps["index_type"].default == "ivfpq" and ps["k_probe"].default == 20


def test_dropin_aliases():
    import sys
    import grafp_amd.dropin as d
    saved = {k: sys.modules.get(k) for k in d._ALIASES}
    try:
        d.install(overwrite=True)
        from encoder.graph_encoder import GraphEncoder          # noqa: F401
        from eval import eval_faiss, get_index, load_memmap_data  # noqa: F401
        from generate import create_db                          # noqa: F401
        from modules.transformations import GPUTransformNeuralfp  # noqa: F401
        from simclr.ntxent import ntxent_loss                   # noqa: F401
        from simclr.simclr import SimCLR                        # noqa: F401
        from test_fp import create_dummy_db, create_fp_db       # noqa: F401
        import grafp_amd.encoder.graph_encoder as real
        assert GraphEncoder is real.GraphEncoder
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_dense_helpers_match_conv_library_semantics():
    """conv1x1 / conv3_stride2 (single-GEMM formulation on (C,B,N)) == F.conv2d on (B,C,N,1)."""
    from torch import nn
    from grafp_amd.encoder._dense import conv1x1, conv3_stride2, from_cbn, to_cbn
    torch.manual_seed(0)
    x = torch.randn(3, 16, 40)
    assert to_cbn(x).shape == (16, 3, 40) and torch.equal(from_cbn(to_cbn(x), x), x)
    assert from_cbn(to_cbn(x.unsqueeze(-1)), x.unsqueeze(-1)).shape == (3, 16, 40, 1)
    for groups in (1, 4):
        conv = nn.Conv2d(16, 24, 1, groups=groups, bias=False)
        got = from_cbn(conv1x1(conv, to_cbn(x)), x)
        np.testing.assert_allclose(got.detach().numpy(), conv(x.unsqueeze(-1)).squeeze(-1).detach().numpy(),
                                   rtol=1e-5, atol=1e-5)
    from _common import CpuOps
    for n in (40, 41):
        xs = torch.randn(2, 16, n)
        down = nn.Conv2d(16, 32, 3, stride=2, padding=1, bias=False)
        with CpuOps():                              # the tap gather is a HIP kernel; its CPU stand-in is test-only
            got = from_cbn(conv3_stride2(down, to_cbn(xs)), xs)
        np.testing.assert_allclose(got.detach().numpy(), down(xs.unsqueeze(-1)).squeeze(-1).detach().numpy(),
                                   rtol=1e-5, atol=1e-5)


def test_dense_part_of_the_model_matches_the_oracle_on_cpu():
    """With the HIP ops swapped for torch/oracle equivalents (TEST-ONLY, _common.CpuOps) the module mirror
    reproduces the oracle's forward AND backward: pins the GEMM / fused-BN / residual wiring, the (C,B,N) layout
    handling and the state-dict mapping without a GPU."""
    from _common import CpuOps, simclr_inputs
    from oracle import model as om
    cfg, model = _model()
    filled = filled_state_dict()
    sd = model.state_dict(); sd.update(filled); model.load_state_dict(sd)
    xi, xj = simclr_inputs()
    with CpuOps():
        model.train()
        h_i, h_j, z_i, z_j = model(xi, xj)
        loss = om.ntxent(z_i, z_j, 0.05)
        loss.backward()
    osd = {k: v.clone() for k, v in filled.items()}
    for k, v in osd.items():
        if v.is_floating_point() and k.rsplit(".", 1)[-1] not in ("running_mean", "running_var"):
            v.requires_grad_(True)
    o = om.simclr_forward(osd, xi, xj, True)
    oloss = om.ntxent(o[2], o[3], 0.05)
    oloss.backward()
    np.testing.assert_allclose(z_i.detach().numpy(), o[2].detach().numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(z_j.detach().numpy(), o[3].detach().numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(h_i.detach().numpy(), o[0].detach().numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(loss.item(), oloss.item(), rtol=1e-5)
    sdm = model.state_dict()
    for k in ("encoder.stem.1.running_mean", "encoder.backbone.7.1.fc1.1.running_var", "encoder.backbone.3.0.fc2.1.running_mean"):
        np.testing.assert_allclose(sdm[k].numpy(), osd[k].detach().numpy(), rtol=1e-4, atol=1e-6)
    assert int(sdm["encoder.stem.1.num_batches_tracked"]) == 2
    P = dict(model.named_parameters())
    gn = max(float(osd[k].grad.norm()) for k in P if P[k].requires_grad)
    rel = [float((P[k].grad - osd[k].grad).norm()) / max(float(osd[k].grad.norm()), 1e-4 * gn)
           for k in P if P[k].requires_grad]
    assert max(rel) < 5e-2 and np.median(rel) < 1e-2, (max(rel), np.median(rel))


def test_sequence_rerank_matches_oracle():
    from grafp_amd.eval import sequence_rerank
    from oracle import retrieval
    rng = np.random.default_rng(0)
    recon = rng.standard_normal((400, 128)).astype(np.float32)
    for sl in (1, 3, 11):
        q = recon[100:100 + sl] + 0.1 * rng.standard_normal((sl, 128)).astype(np.float32)
        I = rng.integers(0, 400, size=(sl, 20))
        I[:, 0] = 100 + np.arange(sl)
        I[0, 5] = -1
        I[-1, 3] = 399                                                   # candidate sequence runs off the end
        pred = sequence_rerank(q, I.copy(), recon, sl)
        J = I - np.arange(sl)[:, None]
        cand = np.unique(J[J >= 0])
        scores = retrieval.sequence_scores(q, recon, cand, sl)
        want = cand[np.argsort(-scores, kind="stable")[:10]]
        assert pred[0] == 100 and np.array_equal(pred, want)


def test_memmap_format_roundtrip(tmp_path):
    from grafp_amd.eval import load_memmap_data
    from grafp_amd.fpdb import _write_memmap
    arr = hash_normalish("host:mm", (37, 128))
    arr[3, 5] = np.nan
    _write_memmap(str(tmp_path / "db"), arr)
    assert os.path.getsize(tmp_path / "db.mm") == 37 * 128 * 4
    assert tuple(np.load(tmp_path / "db_shape.npy")) == (37, 128)
    data, shape = load_memmap_data(str(tmp_path), "db", display=False)
    assert tuple(shape) == (37, 128) and data[3, 5] == 0.0               # NaN -> 0 (eval.py:165)
    ref = arr.copy(); ref[3, 5] = 0.0
    np.testing.assert_array_equal(np.asarray(data), ref)
    assert tuple(load_memmap_data(str(tmp_path), "db", shape_only=True)) == (37, 128)


def test_config_and_util():
    from grafp_amd import util
    cfg = util.load_config()
    ref = dict(fs=16000, n_fft=1024, win_len=1024, hop_len=512, n_mels=64, n_frames=32, peak_stride=2, n_filters=8,
               d=128, h=1024, u=32, tau=0.05, bsz_train=256, overlap=0.9, blur_kernel=[7, 7], arch="grafp")
    assert all(cfg[k] == v for k, v in ref.items())
    assert [util.query_len_from_seconds(s, 0.9, 1.0) for s in (1, 2, 3, 5)] == [1, 10, 20, 40] or \
        [util.query_len_from_seconds(s, 0.9, 1.0) for s in (1, 2, 3, 5)] == [1, 11, 21, 41]
    assert util.override(3, None) == 3 and util.override(3, 5) == 5


def test_augmentation_banks_and_cpu_branch(tmp_path):
    """Recordings are decoded once into zero-padded banks (.npy and PCM .wav, directory / list / array sources);
    a wrong sample rate is refused; without a GPU the transforms themselves refuse to run (no CPU fallback); the
    DataLoader-worker branch (cpu=True) stays an identity crop."""
    import wave
    from grafp_amd.modules.transformations import GPUTransformNeuralfp, load_bank
    from grafp_amd.util import load_config
    cfg = load_config()
    a = (np.sin(np.arange(300) * 0.1) * 0.5).astype(np.float32)
    np.save(tmp_path / "a.npy", a)
    pcm = (np.clip(np.cos(np.arange(500) * 0.05), -1, 1) * 32767).astype("<i2")
    for name, fs in (("b.wav", cfg["fs"]), ("bad.wav", 8000)):
        with wave.open(str(tmp_path / name), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs); w.writeframes(pcm.tobytes())
    bank, starts, lens = load_bank([str(tmp_path / "a.npy"), str(tmp_path / "b.wav")], cfg["fs"])
    assert bank.shape == (800,) and lens.tolist() == [300, 500] and starts.tolist() == [0, 300]     # ragged: no padding
    assert np.array_equal(bank[:300].numpy(), a)
    np.testing.assert_allclose(bank[300:].numpy(), pcm.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError):
        load_bank(str(tmp_path / "bad.wav"), cfg["fs"])
    (tmp_path / "d").mkdir(); np.save(tmp_path / "d" / "x.npy", a)
    assert load_bank(str(tmp_path / "d"), cfg["fs"])[2].tolist() == [300]
    b3 = load_bank(np.ones((3, 7), np.float32), cfg["fs"], max_len=5)
    assert b3[0].shape == (15,) and b3[1].tolist() == [0, 5, 10]
    t = GPUTransformNeuralfp(cfg, str(tmp_path / "d"), np.ones((2, 100), np.float32), train=True)
    assert t.ir_bank.shape == (300,) and t.noise_len.tolist() == [100, 100] and t.noise_start.tolist() == [0, 100]
    with pytest.raises(RuntimeError):
        t.train_transform(torch.zeros(2, 16000))           # CPU tensors: the HIP path refuses, nothing falls back
    t = GPUTransformNeuralfp(cfg, None, None, cpu=True)
    a, b = t(torch.zeros(16000), torch.arange(16010.0))
    assert b.shape == (16000,)


_IMPORT_REFERENCE_SCRIPTS = r'''
import importlib.util, os, sys
sys.dont_write_bytecode = True
REF, ROOT = sys.argv[2], sys.argv[1]
sys.path.insert(0, ROOT)
assert "faiss" not in sys.modules

sys.path.insert(0, REF)                        # the stand-in checkout: its scripts, util.py, modules/data.py
import grafp_amd.dropin as dropin
names = dropin.install()
assert "faiss" in names and "util" not in names and "modules" not in names, names

def load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, fname))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod); return mod

import grafp_amd.eval, grafp_amd.fpdb, grafp_amd.faiss_standin
import grafp_amd.encoder.graph_encoder as ge, grafp_amd.simclr.simclr as sc, grafp_amd.simclr.ntxent as nx
import grafp_amd.modules.transformations as tf

t = load("ref_test_fp", "test_fp.py")          # module level: imports, argparse definitions; main() is not run
assert t.faiss is grafp_amd.faiss_standin and t.faiss.IndexFlatL2 is grafp_amd.ops.FlatL2Index
assert t.eval_faiss is grafp_amd.eval.eval_faiss and t.get_index is grafp_amd.eval.get_index
assert t.load_memmap_data is grafp_amd.eval.load_memmap_data
assert t.GraphEncoder is ge.GraphEncoder and t.SimCLR is sc.SimCLR and t.GPUTransformNeuralfp is tf.GPUTransformNeuralfp
assert t.load_config.__module__ == "util" and sys.modules["util"].__file__.startswith(REF)      # the reference's own
assert t.NeuralfpDataset.__module__ == "modules.data" and sys.modules["modules.data"].__file__.startswith(REF)
assert sys.modules["modules.transformations"] is tf and sys.modules["modules"].transformations is tf

tr = load("ref_train", "train.py")
assert tr.create_fp_db is grafp_amd.fpdb.create_fp_db and tr.create_dummy_db is grafp_amd.fpdb.create_dummy_db
assert tr.eval_faiss is grafp_amd.eval.eval_faiss and tr.ntxent_loss is nx.ntxent_loss
assert tr.SimCLR is sc.SimCLR and tr.GraphEncoder is ge.GraphEncoder and tr.GPUTransformNeuralfp is tf.GPUTransformNeuralfp

g = load("ref_generate", "generate.py")
assert g.GraphEncoder is ge.GraphEncoder and g.SimCLR is sc.SimCLR and g.GPUTransformNeuralfp is tf.GPUTransformNeuralfp

# the reference's OWN eval.py against the stand-in: its module-level GPU plumbing (eval.py:42-46) runs on it
e = load("ref_eval", "eval.py")
assert e.faiss is grafp_amd.faiss_standin
import faiss
opts = faiss.GpuClonerOptions(); opts.useFloat16 = True
assert faiss.index_cpu_to_gpu(faiss.StandardGpuResources(), 0, "index", opts) == "index"
print("reference scripts import through the alias route")
'''


def _reference_standin(root):
    """A stand-in checkout of the reference under `root`, built from tests/golden/reference_imports.json (the project
    imports of its train.py, test_fp.py, generate.py and eval.py, in source order; tests/golden/make_reference_imports.py):
    each script holds exactly those import statements, and the two host-side files the scripts keep their own --
    util.py and modules/data.py -- define the names imported from them."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_imports.json")) as f:
        imports = json.load(f)
    own = {"util": os.path.join(root, "util.py"), "modules.data": os.path.join(root, "modules", "data.py")}
    defined = {m: set() for m in own}
    os.makedirs(os.path.join(root, "modules"))
    open(os.path.join(root, "modules", "__init__.py"), "w").close()
    for fname, stmts in imports.items():
        lines = []
        for module, names in stmts:
            lines.append(f"import {module}" if names is None else f"from {module} import {', '.join(names)}")
            if module in own:
                defined[module].update(n for n in names if n != "*")
        with open(os.path.join(root, fname), "w") as f:
            f.write("\n".join(lines) + "\n")
    for module, path in own.items():
        with open(path, "w") as f:
            f.write("".join(f"def {n}(*args, **kwargs):\n    raise NotImplementedError\n\n\n" for n in sorted(defined[module])))


def test_reference_scripts_import_through_the_alias_route(tmp_path):
    """with grafp_amd.dropin.install() -- which now also registers a `faiss` stand-in -- the reference's
    train.py, test_fp.py, generate.py (and its own eval.py) IMPORT unchanged from a checkout of the reference, and the
    names they bind are this package's: GraphEncoder, SimCLR, ntxent_loss, GPUTransformNeuralfp, eval_faiss, get_index,
    create_fp_db, create_dummy_db, faiss.IndexFlatL2.  util.py and modules/data.py stay the checkout's own host-side
    files.  The checkout is a stand-in with the scripts' recorded import statements (_reference_standin)."""
    import subprocess
    import sys
    ref = str(tmp_path / "reference")
    _reference_standin(ref)
    script = tmp_path / "import_ref.py"
    script.write_text(_IMPORT_REFERENCE_SCRIPTS)
    res = subprocess.run([sys.executable, str(script), ROOT, ref], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600, cwd=str(tmp_path))
    assert res.returncode == 0 and "import through the alias route" in res.stdout, res.stdout[-3000:]


def test_optimizer_refuses_what_the_path_does_not_use():
    """grafp_amd.optim.Adam is torch.optim.Adam with step() on the multi-tensor kernel for what train.py:174 uses (the
    defaults); the options outside the path raise at construction instead of silently running another update, and the
    object keeps torch's state_dict schema (param_groups keys) so that a checkpoint of either class loads into the other."""
    import torch
    from grafp_amd.optim import Adam
    w = torch.nn.Parameter(torch.zeros(4))
    for bad in ({"weight_decay": 1e-2}, {"amsgrad": True}, {"maximize": True}):
        with pytest.raises(NotImplementedError):
            Adam([w], lr=1e-3, **bad)
    opt = Adam([w], lr=3e-4)
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=3e-4)
    assert isinstance(opt, torch.optim.Adam)
    keys = set(ref.state_dict()["param_groups"][0])
    assert set(opt.state_dict()["param_groups"][0]) == keys
    g, h = opt.param_groups[0], ref.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (h["lr"], h["betas"], h["eps"], 0, False)
    w.grad = torch.ones(4)
    with pytest.raises(RuntimeError):                   # a CPU parameter: there is no CPU fallback behind step()
        opt.step()


@pytest.mark.parametrize("order", ["ABAB", "ABBA", "AAA", "ABCCBA"])
def test_deferral_bookkeeping_first_use_of_each_weight_only(order, monkeypatch):
    """ops._may_defer inside defer_wgrad_reduce(): exactly the FIRST gradient of each weight in the block may stay
    unreduced; every later one flushes the queue first and is reduced at once -- also after a flush (A B A B: the flush
    of A's second use must not forget that B was used), so autograd never adds into unreduced memory.  CPU leaf
    tensors under no_grad: the queue stays empty, so a flush launches nothing; flushes are counted."""
    from grafp_amd import ops
    flushes = []
    real = ops.flush_wgrad_reduce                            # counted, and still run: the queue is empty, no launch
    monkeypatch.setattr(ops, "flush_wgrad_reduce", lambda: (flushes.append(1), real()))
    ws = {c: torch.zeros(4, requires_grad=True) for c in "ABC"}
    with torch.no_grad(), ops.defer_wgrad_reduce():
        seen = set()
        for c in order:
            before = len(flushes)
            got = ops._may_defer(ws[c])
            if c in seen:
                assert got is False and len(flushes) == before + 1, (order, c)
            else:
                assert got is True and len(flushes) == before, (order, c)
            seen.add(c)
    assert not ops._WGRAD_SEEN_IDS and ops._WGRAD_PENDING is None


def test_deferral_bookkeeping_survives_nesting_and_existing_grad(monkeypatch):
    """A weight whose .grad was set after its first deferral (a second backward pass inside the block: AccumulateGrad
    would ADD into the unreduced tensor) flushes before it is reduced; nested blocks keep what the outer one saw, and
    only leaving the outermost block forgets it."""
    from grafp_amd import ops
    flushes = []
    real = ops.flush_wgrad_reduce                            # counted, and still run: the queue is empty, no launch
    monkeypatch.setattr(ops, "flush_wgrad_reduce", lambda: (flushes.append(1), real()))
    a, b = torch.zeros(4, requires_grad=True), torch.zeros(4, requires_grad=True)
    with torch.no_grad():
        with ops.defer_wgrad_reduce():
            assert ops._may_defer(a) is True and not flushes
            a.grad = torch.zeros(4)                          # what the first backward pass left behind
            assert ops._may_defer(a) is False and len(flushes) == 1
            with ops.defer_wgrad_reduce():                   # nested: the same bookkeeping
                assert ops._may_defer(b) is True
                assert ops._may_defer(a) is False and len(flushes) == 2
            assert ops._WGRAD_PENDING is not None and ops._WGRAD_SEEN_IDS
            assert ops._may_defer(b) is False and len(flushes) == 3
        assert not ops._WGRAD_SEEN_IDS and ops._WGRAD_PENDING is None
        a.grad = None
        with ops.defer_wgrad_reduce():                       # a new block: first uses again
            assert ops._may_defer(a) is True and ops._may_defer(b) is True
        assert ops._may_defer(a) is True                     # outside any block nothing is tracked
        assert not ops._WGRAD_SEEN_IDS


def test_wgrad_plan_target_only_for_a_deferred_gradient_inside_a_block(monkeypatch):
    """ops._wgrad_plan -> (may_defer, target): inside defer_wgrad_reduce() the first use of a weight may be deferred and is
    produced in place, in what the registered _GRAD_TARGET_OF returns for it; its second use flushes once and gets
    neither; outside any block there is no target; a weight with an existing .grad gets neither."""
    from grafp_amd import ops
    flushes = []
    real = ops.flush_wgrad_reduce                            # counted, and still run: the queue is empty, no launch
    monkeypatch.setattr(ops, "flush_wgrad_reduce", lambda: (flushes.append(1), real()))
    a, b = torch.zeros(4, requires_grad=True), torch.zeros(4, requires_grad=True)
    slices = {id(a): torch.zeros(4), id(b): torch.zeros(4)}
    asked = []
    monkeypatch.setattr(ops, "_GRAD_TARGET_OF", lambda w: (asked.append(id(w)), slices[id(w)])[1])
    with torch.no_grad():
        assert ops._wgrad_plan(a) == (True, None) and not asked          # outside any block: deferrable, never in place
        with ops.defer_wgrad_reduce():
            for w in (a, b):
                may, tgt = ops._wgrad_plan(w)
                assert may is True and tgt is slices[id(w)] and not flushes
            assert ops._wgrad_plan(a) == (False, None) and len(flushes) == 1
            assert ops._wgrad_plan(b) == (False, None) and len(flushes) == 2
            assert asked == [id(a), id(b)]                   # a weight seen before is never asked for a target
        assert ops._wgrad_plan(a) == (True, None) and ops._wgrad_plan(None) == (False, None)
        b.grad = torch.zeros(4)                              # gradient accumulation without zero()
        with ops.defer_wgrad_reduce():
            assert ops._wgrad_plan(b) == (False, None)
            may, tgt = ops._wgrad_plan(a)
            assert may is True and tgt is slices[id(a)] and ops._may_defer(a) is False
        assert ops._wgrad_plan(b) == (False, None)
    assert not ops._WGRAD_SEEN_IDS and ops._WGRAD_PENDING is None and len(asked) == 3


@pytest.mark.parametrize("shape", [(8, 4, 1, 1), (8, 4)])
def test_forward_operand_uses_the_prepared_copy_only_when_it_fits(shape):
    """ops._forward_operand(w, lowp, dtype): a prepared copy of that dtype and of w's element count is used as it is (same
    storage, as (R, -1) rows); a copy of another dtype, of another element count, or none: a fresh cast of w."""
    from grafp_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(shape, generator=g, requires_grad=True)
    want = w.detach().reshape(8, 4).to(torch.bfloat16)
    lowp = w.detach().to(torch.bfloat16)
    got = ops._forward_operand(w, lowp, torch.bfloat16)
    assert got.data_ptr() == lowp.data_ptr() and got.shape == (8, 4) and torch.equal(got, want) and not got.requires_grad
    for other in (w.detach().to(torch.float16), torch.zeros(8, 8, dtype=torch.bfloat16), None):
        got = ops._forward_operand(w, other, torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.shape == (8, 4) and torch.equal(got, want) and not got.requires_grad
        assert other is None or got.data_ptr() != other.data_ptr()
        assert got.data_ptr() != w.data_ptr()
