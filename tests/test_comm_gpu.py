"""GPU: the collectives of the product (lto_comm_* / lto_group_comm_*, RCCL bound at run time).

The GPU box has ONE device, so what runs here is: an RCCL communicator of world size 1 (init, all-gather, all-reduce on a
real ncclComm), the single-process group form on a group that repeats device 0 (partition, halos, per-member plans and
streams, device-resident gather + reduce, bit-equal to an unsharded sweep), and -- only when two GPUs are visible -- two
ranks running the product callable hip_indirect_defect + the native all-gather.  The driver's 8-GPU scaling run exercises
the N > 1 RCCL path through bench.py."""
import ctypes
import os
import socket

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import sharding, synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu
PRM = [MU, DU, TU, 0.05, 1000.0, 1.0, 1.0, 1.0]


def test_rccl_is_bound_and_world1_collectives(gpu_ctx):
    import torch
    assert lto.Comm.available(), "librccl.so.1 could not be loaded"
    uid = lto.Comm.unique_id()
    assert len(uid) == 128
    comm = lto.Comm(gpu_ctx, 1, 0, uid)
    st = lto.current_stream_ptr()
    send = torch.arange(1000, dtype=torch.float64, device="cuda") * 0.5
    recv = torch.full((1, 1000), -1.0, dtype=torch.float64, device="cuda")
    comm.allgather(send, recv, 1000, stream=st)
    buf = send.clone()
    comm.allreduce(buf, 1000, "sum", stream=st)
    buf2 = send.clone()
    comm.allreduce(buf2, 1000, "max", stream=st)
    torch.cuda.synchronize()
    assert torch.equal(recv[0], send) and torch.equal(buf, send) and torch.equal(buf2, send)
    assert comm.rccl_ranks() == 1 and not comm.uses_windows()          # ncclCommCount of the communicator itself
    assert comm.lib.lto_comm_allreduce_dev(comm.handle, None, None, 10, 0) == lto._lib.LTO_ENULL      # misuse: no buffer
    comm.close()


@pytest.mark.parametrize("members", [2, 3])
def test_group_sharded_sweep_with_device_resident_gather_and_decision(gpu_ctx, members):
    """One host process, a group of `members` contexts on device 0: every member sweeps its block of segments with its own
    device-resident plan on its own stream, the defect slabs are all-gathered on the device (lto_group_comm_allgather_dev)
    and the line-search / convergence quantities -- sum(defect.^2) and norm(defect, Inf), indirect.jl:240,331 -- are reduced
    on the device (lto_defect_norms_dev per slab + lto_group_comm_allreduce_dev): nothing crosses PCIe between sweep and
    decision.  Results equal the unsharded sweep bit for bit."""
    import torch
    n = 101
    S = n - 1
    XC, T = synth.indirect_problem(n, seed=7)
    XC, t = XC[:, :, 0], T[:, 0]
    prm = lto.make_params(*PRM)
    integ = lto.integrator(lto.RK4, steps=32)
    d_ref, _ = lto.indirect_defectCalc(XC, t, prm, integ, ctx=gpu_ctx)
    grp = lto.Group([0] * members)
    gc = lto.GroupComm(grp)
    assert not gc.uses_rccl()          # one device repeated: device copies, no RCCL clique
    cmax = sharding.partition(S, members, 0)[1]
    send, recv, norms, plans, keep = [], [], [], [], []
    for k in range(members):
        ln, lt, s0, cnt = sharding.local_nodes(XC, t, members, k)
        ctx = gc.member(k)
        plan = lto.IndirectPlan(ctx, cnt + 1, 1, prm, integ)
        Xd = torch.from_numpy(synth.to_soa_nodes(np.asfortranarray(ln)[:, :, None])).cuda()
        td = torch.from_numpy(np.ascontiguousarray(lt)).cuda()
        slab = torch.zeros(12, cmax, dtype=torch.float64, device="cuda")       # padded to the largest block
        plan.defect(Xd, cnt + 1, td, 1, slab, cmax, stream=gc.stream(k))
        nm = torch.zeros(2, dtype=torch.float64, device="cuda")                  # [sum of squares, max abs] of the slab
        ctx.check(ctx.lib.lto_defect_norms_dev(ctx.handle, gc.stream(k), lto.hotpath._dptr(slab), cmax, 12, cmax, 1,
                                                lto.hotpath._dptr(nm[0:1]), lto.hotpath._dptr(nm[1:2])))
        send.append(slab); recv.append(torch.zeros(members, 12, cmax, dtype=torch.float64, device="cuda"))
        norms.append(nm); plans.append(plan); keep += [Xd, td]
    gc.allgather(send, recv, 12 * cmax)
    ss = [nm[0:1] for nm in norms]; mx = [nm[1:2] for nm in norms]
    gc.allreduce(ss, 1, "sum")
    gc.allreduce(mx, 1, "max")
    gc.synchronize()
    for k in range(members):
        full = np.zeros((12, S))
        for r in range(members):
            s0, cnt = sharding.partition(S, members, r)
            full[:, s0:s0 + cnt] = recv[k][r, :, :cnt].cpu().numpy()
        assert np.array_equal(full, d_ref), "member %d" % k
        assert abs(float(ss[k]) - float((d_ref ** 2).sum())) <= 1e-12 * float((d_ref ** 2).sum())
        assert float(mx[k]) == float(np.abs(d_ref).max())
    for p in plans:
        p.close()
    gc.close()
    grp.close()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, n_nodes, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # launcher only: carries the 128-byte RCCL id
    ctx = lto.Context(rank)
    box = [lto.Comm.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    comm = lto.Comm(ctx, world, rank, box[0])
    XC, T = synth.indirect_problem(n_nodes, seed=5)
    sweep = sharding.hip_indirect_defect(ctx, lto.make_params(*PRM), lto.integrator(lto.RK4, steps=8))     # the product callable
    full = sharding.sharded_defect(sweep, XC[:, :, 0], T[:, 0], world, rank, device=torch.device("cuda", rank), comm=comm)
    torch.cuda.synchronize()
    q.put((rank, full.cpu().numpy()))
    dist.barrier()
    comm.close(); ctx.close()
    dist.destroy_process_group()


def test_two_ranks_product_sweep_plus_native_allgather(gpu_ctx):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 visible GPUs (this box has %d): the world-2 partition logic runs on CPU in "
                    "tests/test_sharding_gloo.py, the N > 1 RCCL path in the driver's multi-GPU bench" % torch.cuda.device_count())
    import torch.multiprocessing as mp
    n_nodes = 64
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_rank_main, args=(r, 2, port, n_nodes, q), daemon=True) for r in range(2)]
    try:
        for p in procs:
            p.start()
        res = dict(q.get(timeout=420) for _ in range(2))
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    for p in procs:
        assert p.exitcode == 0
    XC, T = synth.indirect_problem(n_nodes, seed=5)
    d_ref, _ = lto.indirect_defectCalc(XC[:, :, 0], T[:, 0], lto.make_params(*PRM), lto.integrator(lto.RK4, steps=8), ctx=gpu_ctx)
    for r in (0, 1):
        assert np.array_equal(res[r], d_ref)


# ------------------------------------------------------------------------------------------- two ranks, ONE device
# The N > 1 hand-off of the one-process-per-GPU layout, on the box's single GPU: two PROCESSES, each with its own lto_ctx on
# device 0, exchanging through the window transport (lto_comm_window_*: export -> the launcher gathers the handles -> open;
# IPC-mapped receive windows, push kernel, flag wait on the stream): both collectives cross the process boundary.  (RCCL is not
# asked to put two ranks on one device here: that is not a configuration it supports -- it refuses or stalls in its bootstrap --
# and a stalled bootstrap would hold the whole suite; on distinct devices lto_comm_create is covered by the two-GPU test above
# and by bench.py --gpus N, whose transport selection reports a refusal in the JSON line instead of swallowing it.)

def _shared_device_rank(rank, world, port, n_nodes, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = {"rank": rank}
    try:
        import datetime
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))   # the launcher: carries the window handles
        ctx = lto.Context(0)
        # the window transport
        XC, T = synth.indirect_problem(n_nodes, seed=5)
        S = n_nodes - 1
        cmax = sharding.partition(S, world, 0)[1]

        def exchange(blob):
            got = [None] * world
            dist.all_gather_object(got, blob)
            return got
        comm = lto.Comm.windows(ctx, world, rank, 12 * cmax, exchange)
        out["windows"] = comm.uses_windows()
        prm, integ = lto.make_params(*PRM), lto.integrator(lto.RK4, steps=8)
        ln, lt, s0, cnt = sharding.local_nodes(XC[:, :, 0], T[:, 0], world, rank)
        plan = lto.IndirectPlan(ctx, cnt + 1, 1, prm, integ)
        Xd = torch.from_numpy(synth.to_soa_nodes(np.asfortranarray(ln)[:, :, None])).cuda()
        td = torch.from_numpy(np.ascontiguousarray(lt)).cuda()
        st = lto.current_stream_ptr()
        fulls = []
        for rep in range(3):                      # repeated: both window halves and their reuse
            slab = torch.zeros(12, cmax, dtype=torch.float64, device="cuda")
            recv = torch.full((world, 12, cmax), -7.0, dtype=torch.float64, device="cuda")
            plan.defect(Xd, cnt + 1, td, 1, slab, cmax, stream=st)       # device-resident sweep of this rank's block
            comm.allgather(slab, recv, 12 * cmax, stream=st)
            torch.cuda.synchronize()
            full = np.zeros((12, S))
            for r in range(world):
                r0, rc = sharding.partition(S, world, r)
                full[:, r0:r0 + rc] = recv[r, :, :rc].cpu().numpy()
            fulls.append(full)
        out["full"] = fulls
        # norms of the local slab -> all-reduce (sum, NaN-propagating max); then a NaN planted on rank 1 only
        nm = torch.zeros(2, dtype=torch.float64, device="cuda")
        ctx.check(ctx.lib.lto_defect_norms_dev(ctx.handle, st, lto.hotpath._dptr(slab), cmax, 12, cmax, 1, lto.hotpath._dptr(nm[0:1]), lto.hotpath._dptr(nm[1:2])))
        ss, mx = nm[0:1].clone(), nm[1:2].clone()
        comm.allreduce(ss, 1, "sum", stream=st)
        comm.allreduce(mx, 1, "max", stream=st)
        bad = torch.tensor([float("nan") if rank == 1 else 3.0, 1.0 + rank], dtype=torch.float64, device="cuda")
        comm.allreduce(bad, 2, "max", stream=st)
        torch.cuda.synchronize()
        out["ss"], out["mx"], out["bad"] = float(ss), float(mx), bad.cpu().numpy()
        out["failed"] = comm.failed(stream=st)    # no wait ran out, nobody lost step
        # one stream per window communicator: a collective on another stream is refused, nothing is enqueued
        side = torch.cuda.Stream()
        try:
            comm.allreduce(ss, 1, "sum", stream=ctypes.c_void_p(side.cuda_stream))
            out["other_stream"] = "accepted"
        except lto.LtoError as e:
            out["other_stream"] = "refused: %s" % e
        dist.barrier()
        # A peer that never arrives: rank 0 gathers alone with a short wait limit -- NaN instead of a hang, and the host can see why.
        if rank == 0:
            comm.set_wait_limit(2000)
            lone = torch.full((world, 12, cmax), -7.0, dtype=torch.float64, device="cuda")
            comm.allgather(slab, lone, 12 * cmax, stream=st)
            torch.cuda.synchronize()
            out["lone_all_nan"] = bool(torch.isnan(lone).all())
            out["lone_failed"] = comm.failed(stream=st)
        dist.barrier()                            # nobody unmaps a window a peer may still be pushing into
        plan.close(); comm.close(); ctx.close()
        dist.destroy_process_group()
    except Exception as e:                        # report instead of hanging the parent
        import traceback
        out["error"] = "%s\n%s" % (e, traceback.format_exc())
    q.put(out)


def test_two_processes_share_the_gpu_windows_carry_the_collectives(gpu_ctx):
    import torch.multiprocessing as mp
    n_nodes, world = 64, 2
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_shared_device_rank, args=(r, world, port, n_nodes, q), daemon=True) for r in range(world)]
    res = {}
    try:
        for p in procs:
            p.start()
        for _ in range(world):
            o = q.get(timeout=420)             # a fresh box pages torch in for every spawned interpreter
            res[o["rank"]] = o
        for p in procs:
            p.join(timeout=60)
    finally:                                   # never leave a rank behind (it would also hold the suite's stdout open)
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    for p in procs:
        assert p.exitcode == 0
    for r in range(world):
        assert "error" not in res[r], res[r].get("error")
    XC, T = synth.indirect_problem(n_nodes, seed=5)
    d_ref, _ = lto.indirect_defectCalc(XC[:, :, 0], T[:, 0], lto.make_params(*PRM), lto.integrator(lto.RK4, steps=8), ctx=gpu_ctx)
    for r in range(world):
        assert res[r]["windows"]
        for full in res[r]["full"]:
            assert np.array_equal(full, d_ref), "rank %d" % r
        assert abs(res[r]["ss"] - float((d_ref ** 2).sum())) <= 1e-12 * float((d_ref ** 2).sum())
        assert res[r]["mx"] == float(np.abs(d_ref).max())
        assert np.isnan(res[r]["bad"][0]) and res[r]["bad"][1] == 2.0          # the NaN of rank 1 reaches every rank
        assert res[r]["failed"] is False
        assert res[r]["other_stream"].startswith("refused") and "ONE stream" in res[r]["other_stream"]
    # a gather whose peer never arrives: NaN, not a hang, and lto_comm_status says so (advisor finding, round 3)
    assert res[0]["lone_all_nan"] and res[0]["lone_failed"]


def test_window_transport_world1_and_misuse(gpu_ctx):
    import torch
    comm = lto.Comm.windows(gpu_ctx, 1, 0, 500, lambda blob: [blob])
    st = lto.current_stream_ptr()
    send = torch.arange(500, dtype=torch.float64, device="cuda") * 0.25
    recv = torch.full((1, 500), -1.0, dtype=torch.float64, device="cuda")
    for _ in range(3):
        comm.allgather(send, recv, 500, stream=st)
    part = torch.full((1, 100), -1.0, dtype=torch.float64, device="cuda")
    comm.allgather(send, part, 100, stream=st)                                  # count < max_count
    b = send.clone(); b[3] = float("nan")
    comm.allreduce(b, 500, "max", stream=st)
    torch.cuda.synchronize()
    assert torch.equal(recv[0], send) and torch.equal(part[0], send[:100])
    assert torch.isnan(b[3]) and torch.equal(b[4:], send[4:])
    with pytest.raises(lto._lib.LtoError):
        comm.allgather(send, recv, 501, stream=st)                              # beyond the window
    assert comm.rccl_ranks() == 0 and comm.uses_windows()                       # no RCCL behind a window communicator
    comm.close()


def _run_bench(extra_env, args, timeout=420):
    """bench.py as a child process -> (exit code, its JSON line or None, tail of stderr).  ONE attempt (the rehearsals
    of the N > 1 path used to be retried once, which hid a starvation mode of four processes on one device): a failure is a failure and
    carries the child's stderr.  The line must be the LAST thing on stdout and within the driver's budget."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(extra_env)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    lines = p.stdout.strip().splitlines()
    out = None
    if lines and lines[-1].startswith("{"):
        assert len(lines[-1]) < 6000, "bench line of %d bytes" % len(lines[-1])
        out = json.loads(lines[-1])
    return p.returncode, out, p.stderr[-8000:]


@pytest.mark.parametrize("world", [4])          # (two ranks: test_bench_collective_on_a_side_stream and the c5 case below)
def test_bench_multi_rank_path_runs_with_ranks_sharing_the_device(world):
    """`bench.py --gpus N` WITHOUT a launcher (N = 4: the window transport with more than one peer): it starts
    torch.distributed.run itself (as a child process, before touching the GPU), all ranks take device 0 (LTO_BENCH_SHARE_DEVICE=1), negotiate the window transport, double-buffer the all-gather of the defect
    slabs inside the timed steps, check their slabs and reduce the timing over ranks -- the code path the driver's 8-GPU run takes,
    on the one device this box has."""
    # (1 024 segments per rank: the ranks' kernels share ONE device here, and a rank's collect kernel polls for flags that its
    # peers' push kernels can only raise if they get compute units at the same time; at the contract size four ranks starve one another)
    rc, out, err = _run_bench({"LTO_BENCH_SHARE_DEVICE": "1"}, ["--gpus", str(world), "--steps", "5", "--warmup", "2", "--no-cpu-baseline",
                                                                "--segments", "1024"])
    assert rc == 0 and out is not None, err
    assert out["n_gpus"] == world and out["steps"] == 5 and out["warmup"] == 2
    assert out["config"]["global_segments"] == world * out["config"]["segments_per_gpu"]
    assert out["config"]["collective"] == "windows" and out["config"]["devices_token"] == "shared"
    assert out["config"]["slab_ok"] is True and out["ok"] is True
    assert out["config"].get("rccl_ranks") is None              # RCCL refuses ranks that share a device: only the windows were set up
    assert out["value"] > 0 and out["scaling"] == "weak"


# (c4 with two ranks -- 131 072 segments per rank -- is one of test_gpu_baseline_shapes.py's per-rank batches; every case here is a
# process launch of ~3 s, and the suite has a time budget)
@pytest.mark.parametrize("wl,world,per_rank", [("c4", 4, 64 * 1024), ("c5", 2, 32768)])
def test_bench_sharded_configs_with_ranks_sharing_the_device(wl, world, per_rank):
    """BASELINE configs[3] / [4] through the N > 1 path: `--workload c4` gives every rank 256 / N homotopy levels of 1 024 segments,
    `--workload c5` 65 536 / N segments (ordered lanes after the warm-up sweep) -- a FIXED global size, so the line says "strong" --
    followed by the all-gather of the defect slabs (12 x segments-per-rank doubles per rank) and the slab check.  Ranks share device
    0 here; on the driver's node every rank has its own."""
    rc, out, err = _run_bench({"LTO_BENCH_SHARE_DEVICE": "1"}, ["--workload", wl, "--gpus", str(world), "--steps", "3", "--warmup", "2",
                                                                "--full", "--no-cpu-baseline"])
    assert rc == 0 and out is not None, err
    assert out["n_gpus"] == world and out["scaling"] == "strong"
    assert out["config"]["segments_per_gpu"] == per_rank and out["config"]["global_segments"] == world * per_rank
    assert {"c4": 262144, "c5": 65536}[wl] == out["config"]["global_segments"]
    assert out["config"]["collective"] == "windows" and out["config"]["slab_ok"] is True
    assert out["value"] > 0
    if wl == "c5":
        assert out["adaptive"]["rebalanced"] is True


@pytest.mark.parametrize("mode", ["auto", "side"])
def test_bench_collective_on_a_side_stream(mode):
    """The N > 1 default on distinct devices: the all-gather of step k on a second stream beside the sweep of step k + 1, the wait
    policy (next sweep behind the gather, or only buffer reuse) measured before the timed legs and agreed by all ranks (`auto`),
    or overlap as given (`side`).  Rehearsed here with two ranks on the one device: the window communicator is bound to the side
    stream by the test gather, events order sweep -> gather -> buffer reuse, the slab check passes.  (One launch at a time: a
    launch is three processes with the GPU open -- the launcher's agent and two ranks -- and the box allows six, this one included.)"""
    rc, out, err = _run_bench({"LTO_BENCH_SHARE_DEVICE": "1", "LTO_BENCH_COLLECTIVE_STREAM": mode},
                              ["--gpus", "2", "--steps", "6", "--warmup", "3", "--no-cpu-baseline", "--segments", "1024"])
    assert rc == 0 and out is not None, err
    c = out["config"]
    assert c["collective"] == "windows" and c["stream"] == "side", c
    if mode == "auto":
        pol = c["policy"]
        assert pol["chosen"] in ("serial", "overlap") and pol["serial_ms"] > 0 and pol["overlap_ms"] > 0, c
        assert (pol["chosen"] == "overlap") == (pol["overlap_ms"] < pol["serial_ms"])
    else:
        assert c["policy"] == "overlap", c
    assert c["slab_ok"] is True and out["n_gpus"] == 2 and out["value"] > 0


def test_bench_under_the_launcher_times_both_transports_and_reports_what_rccl_saw():
    """The N > 1 negotiation on the real RCCL back end, as far as one GPU allows: bench.py under torch.distributed.run with one rank
    (LTO_BENCH_FORCE_COLLECTIVE=1: process group "nccl", collective inside every step).  Both of the library's transports are set up,
    pass the test gather and are TIMED before the timed legs; the line names the faster one, both times, and the number of ranks
    RCCL's own communicator reports."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LTO_BENCH_FORCE_COLLECTIVE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    def launch(extra):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--no-configs"]
        return subprocess.Popen(cmd, env=dict(env, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    # (two launches side by side -- two agents and two ranks with the GPU open, five processes with this one, the box allows six:
    # a launch is ~4.5 s of start-up and the suite has a time budget)
    # the N > 1 default on distinct devices: collective on a side stream, wait policy measured, both transports in play
    pa = launch({"LTO_BENCH_COLLECTIVE_STREAM": "auto"})
    # and with the transport named, on the sweep's own stream: RCCL carries the timed legs
    pb = launch({"LTO_BENCH_TRANSPORT": "rccl"})
    try:
        oa, ea = pa.communicate(timeout=420)
        ob, eb = pb.communicate(timeout=420)
    finally:
        for q in (pa, pb):
            if q.poll() is None:
                q.kill()
    assert pa.returncode == 0, ea[-4000:]
    last = oa.strip().splitlines()[-1]
    assert len(last) < 6000
    out = json.loads(last)
    c = out["config"]
    assert c["rccl_ranks"] == 1, c
    tr = c["transports"]
    assert tr["windows_ms"] > 0 and tr["rccl_ms"] > 0 and tr["chosen"] in ("windows", "rccl") and c["collective"] == tr["chosen"], c
    assert (tr["chosen"] == "windows") == (tr["windows_ms"] <= tr["rccl_ms"])
    assert c["stream"] == "side" and c["policy"]["chosen"] in ("serial", "overlap"), c
    assert c["slab_ok"] is True and c["devices_token"] == "distinct" and out["ok"] is True
    assert pb.returncode == 0, eb[-4000:]
    c = json.loads(ob.strip().splitlines()[-1])["config"]
    assert c["collective"] == "rccl" and c["rccl_ranks"] == 1 and c.get("transports") is None, c


def test_bench_transport_set_up_failing_on_one_rank_ends_cleanly_on_all():
    """One rank's window set-up fails (test hook): every rank still issues the same torch.distributed collectives, agrees that the
    transport is unusable, closes nothing a peer may touch before the barrier, and -- ranks sharing a device have no other transport --
    leaves with the same exit code instead of hanging (advisor finding, round 3)."""
    rc, out, err = _run_bench({"LTO_BENCH_SHARE_DEVICE": "1", "LTO_BENCH_FAIL_RANK": "1"},
                              ["--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--segments", "1024"], timeout=300)
    assert rc != 0
    assert out is not None and "no usable transport" in out["error"] and "windows" in out["tried"], err
