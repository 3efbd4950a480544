"""CPU-side tests: plugin boundary, checkpoint surface, C-ABI export list, synthetic inputs, DP glue (gloo, world 2)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import poem_v2_amd as pk
from poem_v2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- plugin boundary ------------------------------------------------------------------------------------------
def test_registry_and_build_from_cfg():
    assert pk.HEAD.get("POEM_Generalized_Head") is pk.POEM_Generalized_Head
    assert pk.TRANSFORMER.get("PtEmbedTRv4") is pk.PtEmbedTRv4
    reg = pk.Registry("toy")

    @reg.register_module()
    class Foo:
        def __init__(self, cfg):
            self.cfg = cfg

    with pytest.raises(KeyError):
        reg.register_module(module=Foo)
    obj = pk.build_from_cfg(pk.CN({"TYPE": "Foo", "A": 1}), reg, data_preset=pk.CN({"X": 2}))
    assert obj.cfg.A == 1 and obj.cfg.DATA_PRESET.X == 2          # kwargs arrive as UPPER-CASE keys
    with pytest.raises(KeyError):
        pk.build_from_cfg(pk.CN({"TYPE": "Nope"}), reg)
    with pytest.raises(TypeError):
        reg.register_module(force=1)


def test_cn_semantics():
    c = pk.CN({"A": {"B": 1}, "L": [{"x": 1}]})
    assert c.A.B == 1 and c.get("Z", 7) == 7 and c.L[0].x == 1
    d = c.clone()
    d.A.B = 2
    assert c.A.B == 1
    c.freeze()
    with pytest.raises(AttributeError):
        c.A.B = 3
    c.defrost()
    c.merge_from_other_cfg(pk.CN({"A": {"C": 5}}))
    assert c.A.B == 1 and c.A.C == 5


def test_head_state_dict_keys_and_checkpoint_loading():
    head = pk.build_head(pk.configs.model_head_cfg("medium"), data_preset=pk.CN({}))
    want = pk.weights.live_key_shapes(256)
    sd = head.state_dict()
    assert list(sd.keys()) == list(want.keys()) or set(sd.keys()) == set(want.keys())
    assert sum(v.numel() for v in sd.values()) == 7209481          # 7.21 M live parameters
    assert head.num_preds == 3
    # a "reference checkpoint": full-model prefixes + dead tensors
    ref = {"module.ptEmb_head." + k: v for k, v in pk.weights.seeded_state_dict(256, seed=5).items()}
    ref["module.ptEmb_head.center_shift_layer.0.weight"] = torch.zeros(799, 799)
    ref["module.ptEmb_head.transformer.pt_metro_encoder.0.embeddings.word_embeddings.weight"] = torch.zeros(8, 256)
    ref["module.img_backbone.conv1.weight"] = torch.zeros(4)
    ignored = head.load_reference_state_dict(ref)
    assert len(ignored) == 3
    assert torch.equal(head.state_dict()["input_proj.weight"], ref["module.ptEmb_head.input_proj.weight"])
    bad = dict(ref)
    bad["module.ptEmb_head.input_proj.bias"] = torch.zeros(3)
    with pytest.raises(ValueError):
        head.load_reference_state_dict(bad)
    del bad["module.ptEmb_head.input_proj.bias"]
    with pytest.raises(KeyError):
        head.load_reference_state_dict(bad)


def test_parametric_head_has_mano_tail_keys():
    head = pk.build_head(pk.configs.model_head_cfg("medium_MANO"), data_preset=pk.CN({}))
    keys = set(head.state_dict().keys())
    assert "transformer.pt_metro_encoder.2.flat_verts.weight" in keys
    assert "transformer.pt_metro_encoder.2.mano_linear.bias" in keys
    assert keys == set(pk.weights.live_key_shapes(256, parametric=True).keys())


def test_no_cpu_fallback():
    head = pk.build_head(pk.configs.model_head_cfg("small"), data_preset=pk.CN({})).eval()
    b = pk.inputs.synthetic_batch([2], seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        head(b["mlvl_feat"], b["img_metas"], b["reference_joints"])
    with pytest.raises(RuntimeError):
        hip.ptr(torch.zeros(3))


def test_head_refuses_training():
    """The HIP head has no backward: the reference's training loop (scripts/train_ddp.py:84, losses at lib/models/POEM.py:363-466
    upstream) must get an error, not a head that silently returns graph-less tensors."""
    head = pk.build_head(pk.configs.model_head_cfg("small"), data_preset=pk.CN({}))
    b = pk.inputs.synthetic_batch([2], seed=0)
    assert head.training
    with pytest.raises(RuntimeError, match="inference-only"):
        head(b["mlvl_feat"], b["img_metas"], b["reference_joints"])                  # train mode, autograd on
    head.eval()
    with pytest.raises(RuntimeError, match="inference-only"):
        head(b["mlvl_feat"].clone().requires_grad_(True), b["img_metas"], b["reference_joints"])   # eval mode, but a gradient is asked for
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(b["mlvl_feat"], b["img_metas"], b["reference_joints"])                  # eval mode, nothing asks for a gradient: past the guard
    head.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        head(b["mlvl_feat"], b["img_metas"], b["reference_joints"])                  # train mode under no_grad (validation inside a training script)


def test_engine_is_rebuilt_when_a_parameter_object_is_replaced(monkeypatch):
    """The engine holds packed copies of the weights and raw pointers into the Parameters: any way a weight can change must
    rebuild it -- in-place edits (version counter), load_state_dict, .data swaps, and a Parameter OBJECT being replaced
    (load_state_dict(assign=True), `module.weight = nn.Parameter(...)`), which a cached list of Parameter objects cannot see."""
    built = []

    class FakeEngine:
        def __init__(self, cfg, weights, *a):
            built.append(float(weights["input_proj.weight"].flatten()[0]))

    monkeypatch.setattr(hip, "Engine", FakeEngine)
    head = pk.build_head(pk.configs.model_head_cfg("small"), data_preset=pk.CN({})).eval()
    head._engine_for("cpu"); head._engine_for("cpu")
    assert len(built) == 1
    with torch.no_grad():
        head.input_proj.weight.mul_(2.0)                                  # in place: version counter
    head._engine_for("cpu")
    assert len(built) == 2
    head.input_proj.weight = torch.nn.Parameter(torch.full_like(head.input_proj.weight, 3.0))     # the object is replaced
    head._engine_for("cpu")
    assert len(built) == 3 and built[-1] == 3.0
    sd = {k: torch.full_like(v, 5.0) for k, v in head.state_dict().items()}
    head.load_state_dict(sd, assign=True)
    head._engine_for("cpu")
    assert len(built) == 4 and built[-1] == 5.0
    head._engine_for("cpu")
    assert len(built) == 4
    # a replaced SUBMODULE (round 5: seen at the very next forward, not within 256): a fresh Conv2d, a parametrization
    import copy
    conv = copy.deepcopy(head.input_proj)
    with torch.no_grad():
        conv.weight.fill_(7.0)
    head.input_proj = conv
    head._engine_for("cpu")
    assert len(built) == 5 and built[-1] == 7.0

    class Twice(torch.nn.Module):
        def forward(self, w):
            return 2.0 * w

    torch.nn.utils.parametrize.register_parametrization(head.input_proj, "weight", Twice())
    head._engine_for("cpu")
    assert len(built) == 6 and built[-1] == 14.0
    head._engine_for("cpu")
    assert len(built) == 6


# ---- C ABI ------------------------------------------------------------------------------------------------------
def _header_functions():
    txt = open(os.path.join(ROOT, "include", "poem_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(poem_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    names = _header_functions()
    assert len(names) >= 25
    L = hip.lib()                                   # loads without a GPU
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/poem_hip.h but not exported"
    assert sorted(hip.SIGNATURES) == names          # the ctypes table mirrors the header one to one
    assert L.poem_abi_version() == hip.ABI_VERSION == 3
    assert L.poem_error_string(-2) == b"workspace too small"


def test_every_option_name_is_documented_in_the_header():
    """poem_set_option's names (csrc/handle.cpp) against the comment of its declaration in include/poem_hip.h: a switch a
    maintainer cannot find in the header does not exist for them."""
    src = open(os.path.join(ROOT, "poem-v2_amd", "csrc", "handle.cpp")).read()
    body = src[src.index("int poem_set_option("):]
    body = body[:body.index("\n}\n")]
    names = sorted(set(re.findall(r'k == "([a-z0-9_]+)"', body)))
    assert len(names) >= 20, names
    hdr = open(os.path.join(ROOT, "include", "poem_hip.h")).read()
    doc = hdr[:hdr.index("int poem_set_option(")]
    doc = doc[doc.rindex("/*"):]
    missing = [n for n in names if f'"{n}"' not in doc]
    assert not missing, missing


def test_library_tensor_table_matches_python():
    import ctypes
    L = hip.lib()
    for model, par in (("small", False), ("medium", False), ("large", False), ("medium", True)):
        C = pk.weights.MODEL_EMBED[model]
        cfg = hip.make_config(C, parametric=par)
        shapes = pk.weights.live_key_shapes(C, parametric=par)
        assert L.poem_num_weight_tensors(ctypes.byref(cfg)) == len(shapes)
        for i, s in enumerate(shapes.values()):
            assert L.poem_weight_tensor_numel(ctypes.byref(cfg), i) == int(np.prod(s))
        assert L.poem_packed_bytes(ctypes.byref(cfg)) > 0
    bad = hip.make_config(100)
    assert L.poem_packed_bytes(ctypes.byref(bad)) == 0
    assert L.poem_num_weight_tensors(ctypes.byref(bad)) < 0
    assert L.poem_gemm(None, 8, None, None, None, 0, None, 8, 1, 8, 8, 0, None) == -1     # argument check, no launch


# ---- synthetic inputs -------------------------------------------------------------------------------------------
def test_synthetic_rig_projects_inside_the_image():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import poem_oracle as po
    b = pk.inputs.synthetic_batch([1, 2, 8, 10], seed=3)
    m = b["img_metas"]
    assert m["cam_view_num"].tolist() == [1, 2, 8, 10]
    offs = np.concatenate([[0], np.cumsum(m["cam_view_num"])])
    for o in offs[:-1]:
        assert torch.equal(m["cam_extr"][o], torch.eye(4))          # view 0 = master = identity
    bps = torch.from_numpy(np.load(os.path.join(hip.ASSETS, "bps.npy")))[0]
    centre = b["reference_joints"][:, 9]
    vs = torch.repeat_interleave(torch.arange(4), torch.tensor([1, 2, 8, 10]))
    uv = po.project_points(bps[None] + centre[:, None], m["cam_intr"], m["cam_extr"], vs)
    assert float(uv.min()) > 0 and float(uv.max()) < 256


# ---- DP glue ----------------------------------------------------------------------------------------------------
def test_shard_ranges_cover_everything():
    from poem_v2_amd.dist import shard_by_views, shard_range
    for n, w in ((32, 8), (33, 8), (5, 8), (64, 3)):
        got = []
        for r in range(w):
            lo, hi = shard_range(n, r, w)
            got += list(range(lo, hi))
        assert got == list(range(n))
    views = np.random.RandomState(5).randint(2, 11, size=64)
    got = []
    for r in range(8):
        lo, hi = shard_by_views(views, r, 8)
        got += list(range(lo, hi))
    assert got == list(range(64))


def pdist_free_port():
    from poem_v2_amd.dist import free_port
    return free_port()


_WORKER = r'''
import os, sys, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
import poem_v2_amd as pk
from poem_v2_amd import dist as pdist
from poem_v2_amd.metrics import MeanEPE, PAEval, Joint3DPCK
rank, local, world = pdist.init_from_env(backend="gloo")
assert world == 2
g = torch.Generator().manual_seed(0)
pred = torch.randn(10, 778, 3, generator=g); gt = torch.randn(10, 778, 3, generator=g)
lo, hi = pdist.shard_range(10, rank, world)
m = MeanEPE("v"); m.feed(pred[lo:hi], gt[lo:hi]); m.reduce()
full = MeanEPE("v"); full.feed(pred, gt)
assert abs(m.result() - full.result()) < 1e-6, (m.result(), full.result())
t = torch.tensor([float(rank + 1)], dtype=torch.float64); pdist.all_reduce_max_(t); assert t.item() == 2.0
# reduce() is non-destructive for every metric: twice in a row, then feed-after-reduce, never counts once per rank.
# (feed() itself is a HIP launch; the accumulators are filled by hand here: rank r holds r+1 samples)
m.reduce(); assert abs(m.result() - full.result()) < 1e-6
pa = PAEval(None, mesh_score=True, device="cpu")
pa.acc += torch.tensor([1.0, 2.0, 3.0, 4.0, 1.0], dtype=torch.float64) * (rank + 1)
for _ in range(2):
    pa.reduce()
    meas = pa.get_measures()
    assert abs(meas["pa_mpjpe"] - 1.0) < 1e-12 and abs(meas["mpvpe"] - 4.0) < 1e-12, meas
    assert pa.acc[4].item() == rank + 1                      # local sums untouched
pck = Joint3DPCK(device="cpu", VAL_MIN=0.0, VAL_MAX=0.02, STEPS=5)
pck.n += (rank + 1); pck.counts[:, 2:] += (rank + 1); pck.sum += 0.01 * (rank + 1)
pck.dists.append(torch.full((rank + 1, 21), 0.03 if rank else 0.01))
for _ in range(2):
    pck.reduce()
    g = pck.get_measures()
    assert abs(g["epe_mean_all"] - 0.01) < 1e-12 and abs(g["pck_curve_per_kp"][0, 2] - 1.0) < 1e-12, g
    assert pck.get_pck_all(0.02) == 1.0                      # a histogram step: from the reduced counts, no collective
    assert abs(pck.get_pck_all(0.017) - 1.0 / 3.0) < 1e-12   # any other threshold: global [hits, total] (1 of 3 samples)
    assert int(pck.n[0]) == rank + 1
# input side (N4): shards are dealt by rank (webdataset.split_by_node), no data-path collective; the union is the epoch
to = pk.inputs
d = sys.argv[2]
if rank == 0:
    for si in range(4):
        pk.wds.write_shard(os.path.join(d, f"Toy_mv_test-{si:06d}.tar"),
                           [to.synthetic_frame(10 * si + i, n_cams=2, raw=(48, 32)) for i in range(3)])
pdist.barrier()
cfg = pk.wds.dataset_cfg(os.path.join(d, "Toy_mv_test-{000000..000003}.tar"))
ds = pk.MultiviewWebDataset(cfg, data_preset=cfg.DATA_PRESET, is_train=False, defer_images=True)
assert len(ds.shards) == 2 and ds.shards == pk.wds.expand_urls(cfg.URLS)[rank::2]
keys = [f["__key__"] for f in ds]
allk = [None, None]; dist.all_gather_object(allk, keys)
assert len(keys) == 6 and sorted(allk[0] + allk[1]) == sorted(f"frame{10 * si + i:06d}" for si in range(4) for i in range(3))
assert not set(allk[0]) & set(allk[1])
pdist.barrier()
if rank == 0: print("DP_OK", m.result())
dist.destroy_process_group()
'''


def test_dp_metric_allreduce_gloo_world2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = str(pdist_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", port, str(script), ROOT, str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "DP_OK" in out.stdout


_WORKER8 = r'''
import os, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from poem_v2_amd import dist as pdist
from poem_v2_amd.metrics import MeanEPE
rank, local, world = pdist.init_from_env(backend="gloo")
assert world == 8
# config c5 as one global batch: 64 ragged samples split by shard_by_views; config c3: 256 samples split by shard_range
views = np.random.RandomState(5).randint(2, 11, size=64)
lo, hi = pdist.shard_by_views(views, rank, world)
spans = [None] * world; dist.all_gather_object(spans, (lo, hi))
assert spans[0][0] == 0 and spans[-1][1] == 64 and all(spans[i][1] == spans[i + 1][0] for i in range(world - 1)), spans
loads = [int(views[a:b].sum()) for a, b in spans]
assert max(hi_ - lo_ for lo_, hi_ in spans) <= 9 and max(loads) <= 1.25 * sum(loads) / world, (spans, loads)
l3, h3 = pdist.shard_range(256, rank, world)
assert (l3, h3) == (32 * rank, 32 * rank + 32)
# the path's only collective: metric sums over the shards == the single-process metric, and reduce() twice changes nothing
g = torch.Generator().manual_seed(0)
pred = torch.randn(64, 778, 3, generator=g); gt = torch.randn(64, 778, 3, generator=g)
m = MeanEPE("v"); m.feed(pred[lo:hi], gt[lo:hi]); m.reduce(); m.reduce()
full = MeanEPE("v"); full.feed(pred, gt)
assert abs(m.result() - full.result()) < 1e-6, (m.result(), full.result())
t = torch.tensor([float(rank)], dtype=torch.float64); pdist.all_reduce_max_(t); assert t.item() == 7.0
pdist.barrier()
if rank == 0: print("DP8_OK", spans)
dist.destroy_process_group()
'''


def test_dp_sharding_and_metric_allreduce_gloo_world8(tmp_path):
    """The N = 8 layout of BASELINE configs[2] / [4] on CPU (gloo): shard_range / shard_by_views cover the batch with balanced,
    contiguous ranges, and the sharded metric equals the single-process one (the world-2 test covers the other metrics)."""
    script = tmp_path / "worker8.py"
    script.write_text(_WORKER8)
    port = str(pdist_free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                          "--master-addr", "127.0.0.1", "--master-port", port, str(script), ROOT],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "DP8_OK" in out.stdout


def test_eval_single_cfg_edits_match_reference():
    """scripts/eval_single.py reproduces the reference script's YAML edits and exp_id (golden: tests/golden/evalcfg.json,
    recorded by running the reference's own main() with the shell-out stubbed)."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_single", os.path.join(root, "scripts", "eval_single.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for g in json.load(open(os.path.join(root, "tests", "golden", "evalcfg.json"))):
        cfg = m.default_cfg()
        vr = m.edit_cfg(cfg, g["dataset"], g["model"], [g["view_min"], g["view_max"]])
        t, h = cfg["DATASET"]["TEST"], cfg["MODEL"]["HEAD"]
        assert t["TARGET"]["URLS"] == g["urls"] and t["EPOCH_SIZE"] == g["epoch_size"]
        assert t["TARGET"]["EPOCH_SIZE"] == g["target_epoch_size"] and t["TARGET"]["VIEW_RANGE"] == g["view_range"]
        assert h["POSITIONAL_ENCODING"]["NUM_FEATS"] == g["num_feats"] and h["EMBED_DIMS"] == g["embed_dims"]
        assert h["TRANSFORMER"]["INPUT_FEAT_DIM"] == g["input_feat_dim"] and h["POINTS_FEAT_DIM"] == g["points_feat_dim"]
        assert h["TRANSFORMER"]["PARAMETRIC_OUTPUT"] == g["parametric"]
        assert f"{g['dataset']}_view_{vr[0]}_{vr[1]}_{g['model']}" == g["exp_id"]
    import pytest
    with pytest.raises(AssertionError):
        m.edit_cfg(m.default_cfg(), "NoSuchSet", "medium", [1, 2])


def test_internal_launcher_declarations_match_their_definitions():
    """csrc/launchers.h declares the kernel launchers of the .hip files as extern "C": such symbols carry no signature, so
    a drifted declaration still links and then corrupts the call (stream read from the wrong slot).  Compare the
    parameter type lists textually."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_abi_decls", os.path.join(root, "tools", "check_abi_decls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    decls, bad = mod.main()
    assert len(decls) >= 30 and not bad, bad


def test_chain_args_ctypes_mirror_matches_chain_h():
    """tests/util.py's ctypes ChainArgs is what test_chain_forms.py hands poem_launch_chain by pointer: a field that drifted
    from csrc/chain.h (order, name or C type) would make the kernels read garbage pointers.  Parse the struct's declarations
    and compare them field by field."""
    import ctypes
    from util import ChainArgs
    src = open(os.path.join(ROOT, "poem-v2_amd", "csrc", "chain.h")).read()
    body = re.search(r"struct ChainArgs\s*\{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.match(r"^((?:const\s+)?[A-Za-z_][\w ]*?)\s*(\*?)\s*([A-Za-z_]\w*)$", decl.split(",")[0].strip())
        assert m, decl
        base, star = m.group(1).replace("const", "").strip(), m.group(2)
        names = [m.group(3)] + [n.strip().lstrip("*").strip() for n in decl.split(",")[1:]]
        for n in names:
            fields.append((n, ctypes.c_void_p if star else ctype[base]))
    assert len(fields) == 39, fields
    assert [(n, t) for n, t in ChainArgs._fields_] == fields


def test_sampling_args_ctypes_mirrors_match_merge_h():
    """tests/util.py's SampleMergeArgs, SampleGroupArgs and MergeTailArgs are what test_sampling_forms.py hands the fused sampling
    launchers by pointer: hold them against csrc/merge.h field by field (order, name, pointer / int / nested struct)."""
    import ctypes
    import util
    src = open(os.path.join(ROOT, "poem-v2_amd", "csrc", "merge.h")).read()
    for name, count in (("SampleMergeArgs", 19), ("SampleGroupArgs", 6), ("MergeTailArgs", 14)):
        body = re.search(r"struct %s\s*\{(.*?)\};" % name, src, re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            m = re.match(r"^((?:const\s+)?[A-Za-z_]\w*)\s*(\*?)\s*([A-Za-z_]\w*)$", decl.split(",")[0].strip())
            assert m, decl
            base, star = m.group(1).replace("const", "").strip(), m.group(2)
            kind = ctypes.c_void_p if star else {"int": ctypes.c_int, "SampleMergeArgs": util.SampleMergeArgs}[base]
            for n in [m.group(3)] + [n.strip() for n in decl.split(",")[1:]]:
                fields.append((n, kind))
        assert len(fields) == count, (name, fields)
        assert [(n, t) for n, t in getattr(util, name)._fields_] == fields, name


def test_bench_refuses_to_report_n_gpus_from_fewer_devices():
    """``python bench.py --gpus N`` without a launcher starts its own ranks; with fewer than N devices it must fail loudly,
    never print a line that claims N GPUs (here: no GPU at all)."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("box has >= 2 GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "POEM_SINGLE_DEVICE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode != 0 and "refusing" in (out.stderr + out.stdout), (out.stdout[-500:], out.stderr[-500:])
    assert "\"n_gpus\"" not in out.stdout


# ---- the plain-Python side of tests/test_gemm_forms.py ---------------------------------------------------------------
def test_gemm_forms_index_maps_are_bijections():
    """The PA / K-image and V-image maps cover their buffer exactly once, the two names of the PA order coincide, and a map
    agrees with the element-by-element statement of the layout comment."""
    import gemm_forms_util as gu
    for rows, cols in ((32, 32), (96, 64), (64, 256)):
        for index in (gu.pa_index, gu.k_image_index, gu.v_image_index):
            idx = index(rows, cols)
            assert idx.shape == (rows, cols)
            assert torch.equal(idx.flatten().sort().values, torch.arange(rows * cols))
        assert torch.equal(gu.pa_index(rows, cols), gu.k_image_index(rows, cols))
    pa, vi = gu.pa_index(64, 32), gu.v_image_index(64, 32)
    for f4 in range(64 * 32 // 4):
        lane, rest = f4 % 64, f4 // 64
        mt, kc = divmod(rest, 32 // 8)
        for e in range(4):
            assert pa[32 * mt + (lane & 31), 8 * kc + 4 * (lane >> 5) + e] == 4 * f4 + e
        g, rest = rest % 4, rest // 4
        mt, vt = divmod(rest, 32 // 32)
        for e in range(4):
            assert vi[32 * mt + 8 * g + 4 * (lane >> 5) + e, 32 * vt + (lane & 31)] == 4 * f4 + e
    assert gu.pa_index(33, 8).max() < gu.image_floats(33, 8) == 64 * 8


def test_gemm_forms_dispatch_mirror_on_the_release_shapes():
    """gemm_forms_util.dispatch for 256 CUs: the decoder's GEMMs at C = 256 (BQ = 25568 rows, 131072 basis-point rows), the
    POEM-huge shapes of the K-slab kernel, and the fall-backs."""
    import gemm_forms_util as gu
    d = lambda *a, **k: gu.dispatch(*a, ncu=256, **k)      # noqa: E731
    assert d(25568, 256, 256) == ("panel", 2, 2, False, False)
    assert d(25568, 1280, 256, act=1, act_split=256, act2=2) == ("panel", 4, 2, True, False)
    assert d(25568, 768, 256) == ("panel", 4, 1, False, False)
    assert d(131072, 1536, 256, seg_cols=256) == ("panel", 4, 2, False, False)
    assert d(131072, 1024, 256, seg_cols=256) == ("panel", 4, 2, False, True)
    assert d(25568, 256, 1024) == ("kslab", 1)
    assert d(33000, 1024, 1024) == ("kslab", 2)
    assert d(25568, 256, 1024, kslab=False) == ("gemm2", 2, 4)
    assert d(799, 256, 256) == ("panel", 1, 1, False, False) and d(799, 256, 256, narrow=False)[:3] == ("panel", 4, 1)
    assert d(257, 256, 1024) == ("gemm2", 1, 2) and d(33, 96, 160) == ("panel", 1, 1, False, False)
    assert d(64, 160, 2048, act=1, act_split=32, act2=2) == ("refuse",)
    assert d(64, 576, 96, act=2, seg_cols=96) == ("refuse",)
    assert gu.gemm2_branch(6085, 1024) == (2, 4) and gu.gemm2_branch(6000, 1024) == (1, 2) and gu.gemm2_branch(77, 96) == (1, 1)
    assert gu.panel_passes(799, 256, ("panel", 1, 1, False, False), 256) == 1
    assert gu.panel_passes(32 * 2049, 32, ("panel", 1, 1, False, False), 256) == 2


def test_gemm_forms_restatements_against_torch():
    """The fp64 / fp32 restatements of test_gemm_forms.py are the operations they claim to be: against torch's linear, gelu, relu and
    layer_norm in float64 (the fp32 ones within fp32 rounding of it); relu_nan keeps a NaN."""
    import gemm_forms_util as gu
    F = torch.nn.functional
    g = torch.Generator().manual_seed(0)
    x, w, b, r = torch.randn(70, 48, generator=g), torch.randn(96, 48, generator=g) / 7, torch.randn(96, generator=g), torch.randn(70, 96, generator=g)
    lin = F.linear(x.double(), w.double(), b.double())
    want = {0: lin, 1: torch.relu(lin), 2: F.gelu(lin)}
    for act in (0, 1, 2):
        assert torch.allclose(gu.gemm_ref(x, w, b, r, act=act), want[act] + r.double(), rtol=0, atol=1e-12)
        assert float((gu.gemm_ref(x, w, b, r, act=act, fp32=True).double() - want[act] - r.double()).abs().max()) < 2e-5
    two = gu.gemm_ref(x, w, b, None, act=1, act_split=32, act2=2)
    assert torch.equal(two[:, :32], want[1][:, :32]) and torch.allclose(two[:, 32:], want[2][:, 32:], rtol=0, atol=1e-12)
    assert torch.isnan(gu.relu_nan(torch.tensor([float("nan"), -1.0, 2.0]))).tolist() == [True, False, False]
    xi, wi = torch.randint(-4, 5, (9, 64), generator=g).float(), torch.randint(-4, 5, (5, 64), generator=g).float()
    assert torch.equal(gu.linear_seq(xi, wi), xi @ wi.T)
    for cols in (32, 96, 256):
        t = torch.randn(7, cols, generator=g) * 3 + 100
        gm, bt = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
        for eps in (1e-12, 1e-5):
            ref = F.layer_norm(t.double(), (cols,), gm.double(), bt.double(), eps)
            assert torch.allclose(gu.layernorm_ref(t, gm, bt, eps), ref, rtol=0, atol=1e-10)
            assert float((gu.layernorm_ref(t, gm, bt, eps, fp32=True).double() - ref).abs().max()) < 1e-4
        wn, bn, base = torch.randn(3, cols, generator=g), torch.randn(3, generator=g), torch.randn(7, 3, generator=g)
        ref = base.double() + F.linear(t.double(), wn.double(), bn.double())
        assert torch.allclose(gu.narrow_ref(t, wn, bn, base), ref, rtol=0, atol=1e-10)
        assert float((gu.narrow_ref(t, wn, bn, base, fp32=True).double() - ref).abs().max()) < 2e-3
        assert torch.allclose(gu.narrow_ref(t, wn), F.linear(t.double(), wn.double()), rtol=0, atol=1e-10)


# ---- tests/conv_forms_util.py: the route mirror of csrc/decode.hip ------------------------------------------------------------
def test_conv_forms_route_literals():
    """conv_forms_util.route on every branch and boundary of decode.hip's launchers, as literal expectations"""
    import conv_forms_util as cu
    r = cu.route
    # 16-row fragments where they pad less, at most five tiles; else 32-row tiles, five at most
    assert [cu.m16(c) for c in (1, 16, 17, 32, 33, 48, 49, 65, 80, 81, 96, 97, 112)] == \
        [True, True, False, False, True, True, False, True, True, False, False, False, False]
    assert r("conv3", 8, 80, 16, 16) == ("lds16", 5, False, 0, False, False) and r("conv3", 8, 96, 16, 16) == ("lds", 3, False, False, False)
    assert r("conv3", 8, 100, 16, 16) == ("lds", 4, False, False, False) and r("conv3", 8, 160, 16, 16, ex=True) == ("lds", 5, False, False, True)
    assert r("conv3", 8, 40, 16, 16, ex=True) == ("lds16", 3, False, 0, False, True) and r("conv3", 8, 9, 4, 64) == ("lds16", 1, False, 0, False, False)
    assert r("conv3", 8, 161, 16, 16) == ("direct", 3, 2, False) and r("conv3", 8, 320, 8, 8) == ("direct", 5, 2, False)
    # the LDS rule: W divides 256, H whole tiles, 8 (TR + 2)(W + 2) staged floats <= 7 x 512 = 3584 (W = 2 would need 4160)
    assert [8 * (256 // w + 2) * (w + 2) for w in (2, 4, 8, 16, 32, 64)] == [4160, 3168, 2720, 2592, 2720, 3168]
    assert not cu.lds_ok(40, 128, 2) and cu.lds_ok(40, 64, 4) and not cu.lds_ok(40, 32, 4) and cu.lds_ok(40, 4, 64) and not cu.lds_ok(40, 6, 64)
    assert not cu.lds_ok(40, 2, 128) and not cu.lds_ok(40, 16, 48) and cu.lds_ok(160, 16, 16) and not cu.lds_ok(161, 16, 16)
    # the direct kernel's tiling: channel tiles 5 | 3 | 2 | 1 by divisibility, two pixel tiles where their count is even
    assert r("conv3", 8, 32, 4, 8) == ("direct", 1, 1, False) and r("conv3", 8, 224, 8, 8) == ("direct", 1, 2, False)
    assert r("conv3", 8, 96, 2, 48, ex=True) == ("direct", 3, 1, True) and r("conv3", 8, 40, 16, 16, 2) == ("direct", 2, 2, False)
    assert r("conv3", 8, 160, 8, 16, 2) == ("direct", 5, 1, False) and r("conv3", 8, 480, 8, 8) == ("direct", 5, 2, False)
    assert r("conv3", 12, 40, 16, 16) is None and r("conv3", 8, 40, 16, 16, 3) is None and r("conv3", 8, 40, 6, 8) is None
    assert r("conv3", 8, 40, 15, 16, 2) is None and r("conv3", 40, 40, 4096, 4096) is None
    # the fused input: the row stager by width and switch, the pinned pipeline for five 32-row tiles
    assert r("upcat", (80, 40), 40, 64, 64) == ("lds16", 3, True, 64, False, False) and r("upcat", (160, 80), 80, 32, 32) == ("lds16", 5, True, 32, False, False)
    assert r("upcat", (80, 40), 40, 64, 64, row_stager=2) == ("lds16", 3, True, 0, False, False)
    assert r("upcat", (160, 80), 80, 32, 32, row_stager=1) == ("lds16", 5, True, 0, False, False)
    assert r("upcat", (16, 8), 16, 16, 16) == ("lds16", 1, True, 0, False, False)
    assert r("upcat", (320, 160), 160, 16, 16) == ("lds", 5, True, True, False) and r("upcat", (320, 160), 160, 16, 16, pin32=0) == ("lds", 5, True, False, False)
    assert r("upcat", (0, 16), 128, 32, 8) == ("lds", 4, True, False, False) and r("upcat", (16, 0), 32, 64, 4) == ("lds", 1, True, False, False)
    for ca, cb, cout, h, w in cu.UPCAT_REFUSED + [(0, 0, 40, 16, 16), (8, 8, 40, 16, 15)]:
        assert r("upcat", (ca, cb), cout, h, w) is None
    # the fused read-out head: three 16-row tiles, W = 64, the row stager, and room in the staging tile (6400 floats)
    assert r("pool_head", (80, 40), 40, 64, 64, j=21) == ("lds16", 3, True, 64, True, False)
    assert [cu.pool_head_fits(*cj) for cj in ((40, 31), (40, 32), (48, 5), (48, 6), (33, 32))] == [True, False, True, False, True]
    assert 40 * 128 + 31 * 41 <= 6400 < 40 * 128 + 32 * 41 and 48 * 128 + 5 * 49 <= 6400 < 48 * 128 + 6 * 49
    for kw in (dict(cout=32), dict(cout=49), dict(cout=64), dict(j=33), dict(j=0), dict(w=32), dict(h=6), dict(row_stager=2), dict(pool_fused=0),
               dict(cin=(0, 40)), dict(cin=(80, 0)), dict(cin=(12, 40))):
        args = dict(cin=(80, 40), cout=40, h=64, w=64, j=21)
        args.update(kw)
        assert r("pool_head", **args) is None, kw
    # the stride-2 family: three shapes, two kernels; persistent blocks per CU by the tile count
    assert r("down2", 40, 80, 64, 64) == ("s2p", 4, 1, 18, 4) and r("down2", 80, 160, 32, 32) == ("s2p", 2, 2, 9, 4)
    assert r("down2", 8, 320, 16, 16) == ("s2p", 1, 4, 5, 4) and r("down2", 8, 320, 16, 16, s2_staging_wave=0) == ("s2", 2, 4, 5)
    assert r("down2", 40, 80, 64, 64, s2_staging_wave=0) == ("s2", 8, 1, 18) and r("down2", 24, 160, 32, 32, s2_staging_wave=0) == ("s2", 4, 2, 10)
    for cin, cout, h, w in cu.DOWN2_REFUSED + [(40, 80, 32, 32), (40, 160, 64, 64)]:
        assert r("down2", cin, cout, h, w) is None
    assert [cu.s2_blocks_per_cu(t, 256) for t in (1, 256, 257, 768, 769, 1024, 1025, 1792, 1793, 2048)] == [3, 3, 3, 3, 2, 2, 3, 2, 3, 3]
    assert cu.s2_blocks_per_cu(1024, 256, 4) == 4 and cu.s2p_grid(960, 16, 256) == (1920, 768) and cu.s2p_grid(3, 64, 256) == (24, 24)
    # feat_in + bilinear x2: 8 x 8 maps, whole 32-channel tiles, (K + C) x 64 floats within 160 KiB
    assert r("up2", 320, 160, 8, 8) == ("conv1x1_up2", 10) and r("up2", 448, 192, 8, 8) == ("conv1x1_up2", 10)
    assert r("up2", 456, 192, 8, 8) is None and r("up2", 40, 48, 8, 8) is None and r("up2", 12, 32, 8, 8) is None and r("up2", 40, 32, 16, 16) is None
    assert r("pool", 64, 0, 2, 2, j=32) == ("pool_head",) and r("pool", 65, 0, 2, 2, j=1) is None and r("pool", 8, 0, 2, 3, j=1) is None
    # the case tables name what they claim
    assert {r("conv3", *c)[1:3] for c in cu.DIRECT_CASES} == {(ct, pt) for ct in (1, 2, 3, 5) for pt in (1, 2)}
    assert all(r("conv3", *c)[0] == "direct" for c in cu.DIRECT_CASES)
    lds = cu.lds_cases()
    assert len(lds) == 75 and all(r("conv3", *c)[0] == ("lds16" if cu.m16(c[1]) else "lds") for c in lds)
    for fam, couts in (("lds", cu.LDS_COUTS), ("lds16", cu.LDS16_COUTS)):
        mine = [c for c in lds if c[1] in couts]
        assert {(c[3], c[2] * c[3] // 256) for c in mine} == {(w, m) for w in cu.LDS_WIDTHS for m in (1, 2, 3)}, fam
        assert {(c[3], c[0]) for c in mine} == {(w, k) for w in cu.LDS_WIDTHS for k in cu.CINS}, fam
    assert {r("conv3", *c)[1] for c in lds if not cu.m16(c[1])} == {1, 2, 3, 4, 5} and {r("conv3", *c)[1] for c in lds if cu.m16(c[1])} == {1, 3, 5}
    up = cu.upcat_cases()
    assert len(up) == 100 and all(r("upcat", (ca, cb), cout, h, w) is not None for ca, cb, cout, h, w in up)
    for cout in cu.UPCAT_COUTS:
        assert {(c[0], c[1]) for c in up if c[2] == cout} == set(cu.CACB) and {(c[3], c[4]) for c in up if c[2] == cout} == set(cu.UPCAT_SHAPES)
    forms = {r("upcat", (ca, cb), cout, h, w, **kw) for ca, cb, cout, h, w in up
             for kw in ({}, dict(row_stager=0), dict(row_stager=1), dict(row_stager=2), dict(pin32=0))}
    assert forms == {("lds", ct, True, False, False) for ct in (1, 2, 3, 4, 5)} | {("lds", 5, True, True, False)} | \
        {("lds16", ct, True, rw, False, False) for ct in (1, 3, 5) for rw in (0, 64, 32)}
    for ca, cb, cout, j, h, taken in cu.POOL_HEAD_CASES:
        assert (r("pool_head", (ca, cb), cout, h, 64, j=j) is not None) == taken
    for k, c, taken in cu.UP2_CASES:
        assert (r("up2", k, c, 8, 8) is not None) == taken


def test_conv_forms_restatements_and_poison():
    """the restatements against torch, and what a poisoned pixel reaches on the CPU: exactly its 3 x 3 neighbourhood"""
    import conv_forms_util as cu
    F = torch.nn.functional
    g = torch.Generator().manual_seed(1)
    x, wt, scale, shift, res = cu.conv_data(g, 2, 8, 5, 6, 8, False)
    y = F.conv2d(x.double(), wt.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    assert torch.equal(cu.conv3_ref(x, wt, scale, shift, torch.float64, res=res), torch.relu(y) + res.double())
    assert torch.equal(cu.conv3_ref(x, wt, scale, shift, torch.float64, res=res, res_pre=1), torch.relu(y + res.double()))
    assert torch.equal(cu.conv3_ref(x, wt, scale, shift, torch.float64, relu=0), y)
    xi, wi, si, hi, ri = cu.conv_data(g, 2, 8, 5, 6, 8, True)
    assert torch.equal(cu.conv3_ref(xi, wi, si, hi, torch.float32, 2, res=ri[:, :, :3, :4]).double(),
                       cu.conv3_ref(xi, wi, si, hi, torch.float64, 2, res=ri[:, :, :3, :4]))
    a, b = cu.upcat_data(g, 2, 8, 8, 6, 8, True)
    up = cu.upcat_ref(a, b, torch.float32)
    assert tuple(up.shape) == (2, 16, 6, 8) and torch.equal(up, up.round()) and torch.equal(up[:, 8:], b)
    assert tuple(cu.upcat_ref(a, None, torch.float64).shape) == (2, 8, 6, 8) and torch.equal(cu.upcat_ref(a[:, :0], b, torch.float32), b)
    for variant in cu.POISONS:
        bad = cu.poison(x, variant)
        assert int((~torch.isfinite(bad)).sum()) == 1 and bool(torch.isfinite(bad[0]).all())
        clean, out = cu.conv3_ref(x, wt, scale, shift, torch.float32, relu=0), cu.conv3_ref(bad, wt, scale, shift, torch.float32, relu=0)
        hit = F.max_pool2d((~torch.isfinite(bad)).any(dim=1, keepdim=True).float(), 3, 1, 1).bool().expand_as(out)
        assert torch.equal(~torch.isfinite(out), hit) and torch.equal(out[~hit], clean[~hit])
    hw, hb = torch.randn(3, 5, generator=g), torch.randn(3, generator=g)
    yn = cu.poison(y.float(), "nan00")
    head = cu.head_ref(yn, hw, hb, torch.float32)
    assert bool(head[1, :, 0, 0].isnan().all()) and int(head.isnan().sum()) == 3
    assert torch.allclose(cu.head_ref(y, hw, hb, torch.float64),
                          torch.sigmoid(F.conv2d(F.max_pool2d(y, 2, 2), hw.double()[:, :, None, None], hb.double())), rtol=0, atol=1e-12)
    xk, wk, bk = torch.randn(2, 8, 8, 8, generator=g), torch.randn(32, 8, generator=g), torch.randn(32, generator=g)
    low = F.interpolate(torch.einsum("oc,nchw->nohw", wk.double(), xk.double()) + bk.double().view(1, -1, 1, 1), scale_factor=2, mode="bilinear")
    assert torch.allclose(cu.up2_ref(xk, wk, bk, torch.float64), low, rtol=0, atol=1e-12)      # the 1x1 convolution commutes with it


def _decode_stage_forms():
    """(what, form) of every launch the decoders make, by the tables of poem_v2_amd.decode (no device needed)"""
    import conv_forms_util as cu
    from poem_v2_amd import decode as dc
    out = []
    f = dc.FEAT_SIZES["HRNet"]
    for i, side in enumerate((64, 32, 16)):
        out.append((f"HRNet feat_delayer.{i}", cu.route("down2", f[i], f[i + 1], side, side)))
        out.append((f"HRNet feat_delayer.{i} direct", cu.route("conv3", f[i], f[i + 1], side, side, 2)))
    out.append(("HRNet feat_in", cu.route("up2", f[3], f[2], 8, 8)))
    for i, side in enumerate((16, 32, 64)):
        out.append((f"HRNet uv_delayer.{i}", cu.route("upcat", (f[3 - i], f[2 - i]), f[2 - i], side, side)))
        out.append((f"HRNet uv_delayer.{i} two launches", cu.route("conv3", f[3 - i] + f[2 - i], f[2 - i], side, side)))
    out.append(("HRNet uv_delayer.2 + uv_out", cu.route("pool_head", (f[1], f[0]), f[0], 64, 64, j=dc.NUM_JOINTS)))
    out.append(("HRNet uv_out", cu.route("pool", f[0], 0, 64, 64, j=dc.NUM_JOINTS)))
    for name in ("resnet18", "resnet34", "resnet50"):
        f = dc.FEAT_SIZES[name]
        for h0, w0 in ((8, 8), (4, 8)):
            for i in range(3):
                ca, cb, cout, h, w = f[3 - i], f[2 - i], f[2 - i], h0 << (i + 1), w0 << (i + 1)
                if ca + cb > dc.K_SPLIT:           # _SplitConv3x3: groups of at most K_SPLIT channels, the last one through poem_conv3x3_ex
                    spans = [min(c0 + dc.K_SPLIT, ca) - c0 for c0 in range(0, ca, dc.K_SPLIT)] + \
                        [min(c0 + dc.K_SPLIT, cb) - c0 for c0 in range(0, cb, dc.K_SPLIT)]
                    for k, cin in enumerate(spans):
                        out.append((f"{name} stage {i} group {k}", cu.route("conv3", cin, cout, h, w, ex=k + 1 == len(spans))))
                    continue
                form = cu.route("upcat", (ca, cb), cout, h, w)
                out.append((f"{name} stage {i} {h}x{w}", form if form is not None else cu.route("conv3", ca + cb, cout, h, w)))
                out.append((f"{name} stage {i} {h}x{w} two launches", cu.route("conv3", ca + cb, cout, h, w)))
            if f[0] <= 64:
                out.append((f"{name} uv_out", cu.route("pool", f[0], 0, h0 << 3, w0 << 3, j=dc.NUM_JOINTS)))
    return out


def test_every_caller_shape_lands_on_a_tested_conv_form():
    """every conv3 / down2 launch of the HRNet-W40 and ResNet-18/34/50 plans and every stage of both decoder branches maps
    through the route mirror to a form tests/test_conv_forms.py has a case for: a new caller shape on an untested form fails here"""
    import conv_forms_util as cu
    from poem_v2_amd import backbone as bb
    from poem_v2_amd import resnet as rn
    tested = cu.tested_forms()
    assert len(tested) == 8 * 2 + 5 * 2 + 3 * 2 + 6 + 9 + 1 + 6 + 2, sorted(tested)
    seen = set()
    plans = [("hrnet", bb.HipPlan(2, h, w)) for h, w in ((256, 256), (128, 256))]
    plans += [(f"resnet{v}", rn.ResNetPlan(2, h, w, v)) for v in (18, 34, 50) for h, w in ((256, 256), (128, 256))]
    for name, plan in plans:
        for op in plan.ops:
            if op["kind"] == "conv3":
                form = cu.route("conv3", op["in"].c, op["out"].c, op["in"].h, op["in"].w, op["stride"], ex=True)
            elif op["kind"] == "down2":
                form = cu.route("down2", op["in"].c, op["out"].c, op["in"].h, op["in"].w)
            else:
                continue
            assert form is not None and form in tested, (name, op["conv"], form)
            seen.add(form)
    for what, form in _decode_stage_forms():
        assert form is not None and form in tested, (what, form)
        seen.add(form)
    print(f"{len(seen)} of {len(tested)} tested forms are in use by a caller")
    assert ("lds16", 3, True, 64, True, False) in seen and ("s2p", 1, 4, 5, 4) in seen and ("conv1x1_up2", 10) in seen
