"""CPU-only checks of the host logic and of the C-ABI library (load + symbols; no compute calls without a GPU)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


def test_library_loads_and_exports_every_declared_symbol():
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    declared = set(re.findall(r"\b(ishap_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/ishap.h but not exported"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    assert L.ishap_version() >= 3        # 2: ishap_mesh_smooth(..., scratch, scratch_bytes, stream); 3: ishap_step_coefs rng fields


def test_hot_kernels_use_no_scratch():
    """Code-object metadata of the built library (tools/kernel_meta.py; no GPU needed): every kernel of a guided step's
    conv / GEMM / attention / elementwise classes must have a private segment of 0 bytes.  Round 6 lost 3 % per edit to an
    argument-struct layout change that made the compiler keep four dwords of `IgemmArgs` in scratch (an s_load + wait + scratch
    store at kernel entry of every LDS-DMA convolution) -- no warning, no test noticed.  Known exceptions, listed so that a new
    one is a decision: the group-local GroupNorm kernels (an unused 20 byte reservation in one VEC = 1 form, real
    spills in the rarely launched VEC = 4 / 8 forms whose 1024-thread launch bound caps them at 128 VGPRs; the hot VEC = 2 forms are held to zero below), the 64-pixel skinny
    GEMM form, and the decoder (256 VGPRs + 20 bytes)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    assert len(ks) > 100
    allowed = ("gn_local_kernel", "gn_bwd_local_kernel", "igemm_skinny_kernelILi4", "triplane_decode_kernel")
    bad = {n: k[".private_segment_fixed_size"] for n, k in ks.items()
           if k.get(".private_segment_fixed_size", 0) != 0 and not any(a in n for a in allowed)}
    assert not bad, bad
    hot = [n for n in ks if "igemm2_kernel" in n or "igemm4_kernel" in n]
    assert len(hot) >= 15 and all(ks[n].get(".private_segment_fixed_size", 0) == 0 for n in hot)
    # the VEC = 2 forms of the group-local GroupNorm are the ones a guided step launches ~110 times: zero since round 6 (their first-unit
    # operands moved to inline-asm loads); the VEC = 4 forms' inline-asm path was left out because it spilled (norm_local.hip, PF)
    hot_gn = [n for n in ks if "gn_local_kernelILi2" in n or "gn_bwd_local_kernelILi2" in n]
    assert len(hot_gn) >= 8 and all(ks[n].get(".private_segment_fixed_size", 0) == 0 for n in hot_gn), \
        {n: ks[n].get(".private_segment_fixed_size", 0) for n in hot_gn}


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "ishapediting_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b|oracle/|ref_cpu", src, re.M), \
                    f"{f} reaches into the oracle"


@pytest.mark.parametrize("steps", [10, 40, 200, 256, 1000])
def test_host_schedule_tables_bit_exact(gold, steps):
    from ishapediting_amd.gaussian_diffusion import create_gaussian_diffusion
    g = gold("g1_schedules")
    d = create_gaussian_diffusion(timestep_respacing=str(steps))
    assert d.timestep_map == g[f"T{steps}_timestep_map"].tolist()
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
              "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        np.testing.assert_array_equal(getattr(d, k), g[f"T{steps}_{k}"])


def test_resize_feat_align_and_offsets_match_reference(gold):
    from ishapediting_amd.drag_utils import feat_channel_map, make_offsets, resize_feat_align
    g = gold("g3_primitives")
    for c in (512, 64, 96):
        out = resize_feat_align(T(g[f"rfa_in_{c}"]))
        np.testing.assert_array_equal(out.numpy(), g[f"rfa_out_{c}"])
    cm = feat_channel_map(512)
    assert cm.shape == (3, 170) and cm[0, 0] == 0 and cm[1, 0] == 85 and cm[0, 85] == 256 and cm.max() == 510
    np.testing.assert_array_equal(make_offsets(2, "cpu").numpy(), g["offsets_r2"])


def test_unet_spec_matches_full_reference_tree(gold):
    from ishapediting_amd.unet_spec import build_spec, full_config
    spec = build_spec(full_config())
    assert [b.cout for b in spec.output_blocks][8] == 512 and spec.output_blocks[8].res_out == 64   # the drag tap
    assert len(spec.input_blocks) == 15 and len(spec.output_blocks) == 15


def test_get_args_defaults_and_no_argv_capture():
    from ishapediting_amd.drag_utils import get_args
    a = get_args()
    assert (a.num_steps, a.w_time, a.feat_layer, a.shape_resolution, a.image_size) == (200, 170, 8, 256, 128)
    assert a.use_fp16 and a.learn_sigma and a.timestep_respacing == "200"


def _worker(rank, world, port, n_edits, q):
    import torch.distributed as dist
    from ishapediting_amd.parallel import gather_volumes, shard_edits
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    mine = shard_edits(n_edits, world, rank)
    vols = [torch.full((4, 4, 4), float(i)) for i in mine]
    out = gather_volumes(vols, n_edits, dst=0)
    if n_edits == world:
        # bench.py's form: the shape is known on every rank and rank 0 reuses its receive buffers
        recv = [torch.empty((4, 4, 4)) for _ in range(world)] if rank == 0 else None
        out2 = gather_volumes(vols, n_edits, dst=0, full_shape=(4, 4, 4), recv=recv)
        if rank == 0:
            assert all(torch.equal(a, b) for a, b in zip(out, out2)) and out2[0] is recv[0]
    if n_edits < world:
        # a rank that owns NO edit must still take part when the shape is passed explicitly (it used to raise
        # AttributeError on `None.device` while the other ranks waited in dist.gather)
        out3 = gather_volumes(vols, n_edits, dst=0, full_shape=(4, 4, 4))
        if rank == 0:
            assert len(out3) == n_edits and all(torch.equal(a, b) for a, b in zip(out, out3))
    if rank == 0:
        q.put([float(v[0, 0, 0]) for v in out])
    dist.barrier()
    dist.destroy_process_group()


def _sample_worker(rank, world, port, num_samples, q):
    import torch.distributed as dist
    from ishapediting_amd.image_sample import gather_samples
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    # fake per-rank batches [2, C=3, 4, 5]: value = 100 * rank + 10 * batch index + channel
    b = torch.arange(2).reshape(2, 1, 1, 1) * 10.0 + torch.arange(3).reshape(1, 3, 1, 1) + 100.0 * rank
    arr = gather_samples(b.expand(2, 3, 4, 5).contiguous(), num_samples)
    q.put((rank, arr.shape, arr[:, 0, 0, :].tolist()))
    dist.destroy_process_group()


@pytest.mark.parametrize("num_samples", [3, 4, 9])
def test_noise2shape_gather_tail_world_size_2_gloo(num_samples):
    """image_sample.py:188-197 of the reference: NHWC permute, all_gather in RANK order, concatenate, cut to num_samples
    (3: the cut falls inside rank 1's batch; 9: more than the two ranks produced -- everything is kept)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sample_worker, args=(r, 2, port, num_samples, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = min(num_samples, 4)
    want = [[100.0 * (i // 2) + 10.0 * (i % 2) + c for c in range(3)] for i in range(4)][:n]
    for rank, shape, rows in got:                      # all_gather: EVERY rank holds the full, ordered result
        assert tuple(shape) == (n, 4, 5, 3) and rows == want


def test_noise2shape_gather_tail_single_process():
    from ishapediting_amd.image_sample import gather_samples
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    arr = gather_samples(x, 1)
    assert arr.shape == (1, 4, 5, 3) and np.array_equal(arr[0], x[0].permute(1, 2, 0).numpy())


@pytest.mark.parametrize("n_edits", [1, 2, 3, 4])
def test_gather_volumes_world_size_2_gloo(n_edits):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_edits, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == [float(i) for i in range(n_edits)]


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback: without libishap_hip.so the binding raises, and so does constructing a model on the CPU."""
    from ishapediting_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libishap_hip.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()
    monkeypatch.undo()
    from ishapediting_amd.unet import UNetModel
    from ishapediting_amd.unet_spec import tiny_config
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        UNetModel(tiny_config(1), torch.device("cpu"))


def test_an_older_build_is_refused_with_the_required_abi(monkeypatch):
    from ishapediting_amd import _lib
    have = _lib.lib().ishap_version()
    assert have == _lib.ABI
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI", have + 1)
    with pytest.raises(RuntimeError, match=rf"older build \(ABI {have} < {have + 1}\): rebuild"):
        _lib.lib()


def test_need_gpu_messages(monkeypatch):
    """the three checks it replaced: mesh.py's per function, metrics.py's for a device left open, render.py's"""
    from ishapediting_amd import _lib, mesh, metrics, render
    tail = " on the GPU (libishap_hip.so); there is no CPU fallback"
    host = torch.zeros((4, 3))
    with pytest.raises(RuntimeError) as e:
        _lib.need_gpu(host, "extract_surface")
    assert str(e.value) == "extract_surface runs" + tail
    with pytest.raises(RuntimeError) as e:
        mesh.cloud_areas(host, 2)
    assert str(e.value) == "cloud_areas runs" + tail
    with pytest.raises(RuntimeError) as e:
        render.render_arrays(host, torch.zeros((0, 3), dtype=torch.int32), render.Camera((0.0, 0.0, 3.0)), 4, 4)
    assert str(e.value) == "render runs" + tail
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        metrics.device_mesh((np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)))
    assert str(e.value) == "mesh metrics run" + tail
    assert _lib.need_gpu("cuda:1", "anything") == torch.device("cuda", 1)        # a named device is taken as it is


def test_tensor_coerces_host_inputs_and_keeps_conforming_ones():
    from ishapediting_amd import _lib
    t = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    assert _lib.tensor(t, torch.float32).data_ptr() == t.data_ptr()
    assert _lib.tensor(t, torch.float32, shape=(-1, 3)).data_ptr() == t.data_ptr()
    assert _lib.tensor(t.requires_grad_(), torch.float32).requires_grad is False
    flat = _lib.tensor(t.detach(), torch.float32, shape=(-1,))
    assert tuple(flat.shape) == (12,) and flat.data_ptr() == t.data_ptr()
    for x in ([[0.1, 0.2, 0.3]], np.array([0.1, 0.2, 0.3]), (0.1, 0.2, 0.3)):          # what numpy.asarray takes
        got = _lib.tensor(x, torch.float32, shape=(-1, 3))
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3) and got.is_contiguous()
        assert np.array_equal(got.numpy(), np.array([[0.1, 0.2, 0.3]], np.float32))
    i = _lib.tensor(np.array([[3, 1, 2]], np.int64), torch.int32)
    assert i.dtype == torch.int32 and i.tolist() == [[3, 1, 2]]
    col = _lib.tensor(t.detach()[:, 1], torch.float64)
    assert col.dtype == torch.float64 and col.is_contiguous() and col.tolist() == [1.0, 4.0, 7.0, 10.0]


def test_visualize_mirrors_the_reference_signatures():
    """triplane_decoder/visualize.py:36,76,108: same parameter names, order and defaults (SURVEY 8b keeps these callable)."""
    import inspect
    from ishapediting_amd import visualize
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(visualize.create_obj) == [("model", E), ("obj_idx", E), ("res", 128), ("max_batch_size", 50000),
                                         ("output_path", "output.obj")]
    assert sig(visualize.create_obj_o3d) == [("model", E), ("obj_idx", E), ("res", 128), ("max_batch_size", 50000)]
    assert sig(visualize.main)[:2] == [("args", None), ("feature", None)]
    a = visualize.build_parser().parse_args(["--output", "o.obj"])
    assert a.res == 128 and a.input is None and a.model_path.endswith(".pt")


def test_mesh_arrays_reads_any_object_with_vertices_and_triangles():
    """train_triplane(mesh=<open3d TriangleMesh>) (main.py:447-451): the device route takes the arrays with np.asarray."""
    from types import SimpleNamespace
    from ishapediting_amd.mesh import mesh_arrays
    m = SimpleNamespace(vertices=[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], triangles=[[0, 1, 2]])
    v, t = mesh_arrays(m)
    assert v.dtype == np.float32 and v.shape == (3, 3) and t.dtype == np.int32 and t.shape == (1, 3)
    v2, t2 = mesh_arrays((torch.tensor(m.vertices), torch.tensor(m.triangles)))
    assert np.array_equal(v, v2) and np.array_equal(t, t2)


def test_bench_counts_gpus_without_loading_hip(monkeypatch):
    """bench.py's spawning parent must not initialise the GPU: the count comes from sysfs and *_VISIBLE_DEVICES."""
    import bench
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2")
    n = bench.visible_gpu_count()
    assert n is not None and n <= 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert bench.visible_gpu_count() == 0


def test_bench_plain_run_leaves_the_side_legs_to_full():
    """A plain bench run times the headline only; the legs reported next to it, and the profile files they write, need --full."""
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert not a.full
    assert bench.parse_args(["--full", "--no-c2", "--shape-profile", "s.csv"]).full
    for opt in ("--shape-profile", "--c4-shape-profile"):
        with pytest.raises(SystemExit):
            bench.parse_args([opt, "s.csv"])


def test_philox_restatement_known_answers():
    """Random123's known-answer vectors for philox4x32-10 pin the test-side generator (tests/helpers.py) that the step kernel's
    in-launch noise is compared with on the GPU (test_gpu_parity.py::test_step_draws_its_own_noise)."""
    from tests.helpers import philox4x32_10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10([np.array([v]) for v in ctr], key)
        assert tuple(int(g[0]) for g in got) == want


def test_product_sources_hold_no_probe_code_and_tools_set_only_live_switches():
    """The library's sources are the product only.  (1) Every preprocessor conditional in csrc/ and include/ is an include guard, a
    test of __HIP_DEVICE_COMPILE__ / __HIPCC__ / __cplusplus, or the one ISHAP_STAMPS switch of csrc/stamps.h: ablations and frozen
    knobs do not live there (a probe is a patch under tools/experiments/probes/, applied to a copy by tools/build_variant.sh).
    (2) One file of csrc/ reads the environment: the switch table.  (3) Every ISHAP_* variable a file under tools/ assigns is a
    row of that table, a switch of the Python package or the bench's own -- a sweep of a variable nobody reads reports "flat"
    for any value.  Patches the experiments README lists as historical (they apply to older commits) are exempt, by name."""
    csrc = os.path.join(ROOT, "ishapediting_amd", "csrc")
    files = [os.path.join(d, f) for d in (csrc, os.path.join(ROOT, "include")) for f in sorted(os.listdir(d))
             if os.path.isfile(os.path.join(d, f))]
    assert len(files) > 30
    bad, stamp_tests, env_readers = [], [], []
    for path in files:
        lines = open(path).read().split("\n")
        if "getenv" in "\n".join(lines) and path.startswith(csrc):
            env_readers.append(os.path.basename(path))
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if not m:
                continue
            names = set(re.findall(r"[A-Za-z_]\w*", m.group(2).split("//")[0])) - {"defined"}
            guard = m.group(1) == "ifndef" and len(names) == 1 and re.match(r"\s*#\s*define\s+%s\s*$" % next(iter(names)), lines[i + 1])
            if names == {"ISHAP_STAMPS"} and os.path.basename(path) == "stamps.h":
                stamp_tests.append(i)
            elif not guard and not (len(names) == 1 and names <= {"__HIP_DEVICE_COMPILE__", "__HIPCC__", "__cplusplus"}):
                bad.append(f"{os.path.relpath(path, ROOT)}:{i + 1}: {line.strip()}")
    assert not bad, "\n".join(bad)
    assert len(stamp_tests) == 1
    assert len(env_readers) == 1, env_readers
    table_src = open(os.path.join(csrc, env_readers[0])).read()
    table = set(re.findall(r'^\s*\{"(ISHAP_[A-Z0-9_]+)",\s*-?\d+,\s*"[^"]+"\},?$', table_src, re.M))
    assert len(table) == 18 and "ISHAP_GN_SPIN_LIMIT" in table, sorted(table)
    # every name the sources pass to the helper is a row (the helper aborts otherwise; this finds it without running the path)
    asked = set()
    for path in files:
        asked |= set(re.findall(r'ishap_switch\("(\w+)"', open(path).read()))
    assert asked == table, asked ^ table
    allowed = table | {"ISHAP_FUSED_UPDATE", "ISHAP_OVERLAP_TAIL", "ISHAP_STEP_RNG", "ISHAP_BENCH_CPU_THREADS"}
    historical = {"fixup8_conv_splitk_groupnorm.patch", "tiled_weights.patch"}
    readme = open(os.path.join(ROOT, "tools", "experiments", "README.md")).read()
    for h in historical:
        assert re.search(r"%s.*historical" % re.escape(h), readme), f"{h} is not listed as historical in tools/experiments/README.md"
    dead = []
    for d, _, fs in os.walk(os.path.join(ROOT, "tools")):
        for f in fs:
            if f in historical or f.endswith((".pyc", ".so")):
                continue
            for name in re.findall(r"(ISHAP_[A-Z0-9_]+)=", open(os.path.join(d, f), errors="replace").read()):
                if name not in allowed:
                    dead.append(f"{os.path.relpath(os.path.join(d, f), ROOT)}: {name}")
    assert not dead, "\n".join(sorted(set(dead)))
