"""Benchmark: device-resident WebSocket frame decode (unmask + UTF-8 validation)
on MI355X, one process per GPU, sessions sharded across GPUs with no collective.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config north|1|3] [--frames F] [--payload P]
                  [--full] [--dump-outputs DIR]

A step = one pass of the decode pipeline (libwsgpu's HIP kernels) over one batch
of F synthetic masked frames per GPU resident in HBM.  Default workload: the
north-star 1-GPU case, 1 M x 4 KiB masked TEXT frames (valid UTF-8, ~70 % ASCII
bytes) in 1024 sessions, validation on.  Prints ONE JSON line (rank 0).

A plain run sets up, warms up, times the K steps and prints the headline line.
--full adds every other measurement to that line: the per-kernel breakdown, the
copy ceiling, the validator stage, the host->device->host lines, the secondary
BASELINE configs and the CPU baselines.  --dump-outputs DIR writes the last timed
step's outputs as .npy files, the same from run to run with the same arguments.

--gpus N > 1 without a torch.distributed environment starts N rank processes
itself (torch.distributed.run, 127.0.0.1) before anything touches a GPU and
exits with their status; under a launcher, --gpus must equal WORLD_SIZE.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import shutil
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import benchsupport  # noqa: E402  (synthetic batches + copy ceiling; loads libwsbench.so on first use)

METRIC = "WebSocket frame decode GiB/s device-resident at 1/2/4/8 MI355X; % HBM peak"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s)

# per-GPU workloads of BASELINE.json (configs[2] and configs[4] are measured as extra
# lines of the N=1 run; configs[0] needs a JDK)
CONFIGS = {
    # north star: unmask + UTF-8 of 1 M x 4 KiB masked TEXT frames at 1 GPU
    "north": dict(frames=1 << 20, payload=4096, sessions=1024, binary=False),
    # configs[1]: 1 M masked BINARY frames, 1 KiB payload, 256 sessions (unmask only)
    "1": dict(frames=1 << 20, payload=1024, sessions=256, binary=True),
    # configs[3]: 64 M x 4 KiB sharded by session over 8 GPUs = 8 M frames per GPU
    # (weak scaling: the per-GPU shard is fixed at every N; 64 M frames do not fit one GPU)
    "3": dict(frames=8 << 20, payload=4096, sessions=1024, binary=False),
}



# flushes the bench lines keep in flight: WSG_BATCHER_MAX_INFLIGHT (snf4j_amd._lib, 4; checked
# equal in tests/test_bench_cli.py); WSG_BENCH_INFLIGHT for A/B runs against builds with another depth
BATCHER_MAX_INFLIGHT = int(os.environ.get("WSG_BENCH_INFLIGHT", "4"))


def apply_tuning(ctx):
    """A/B runs (scripts/ab_env.sh): WSG_TUNE_<NAME>=<value> in the bench's environment
    sets the context switch wsg_set_tuning(<NAME>) — the harness reads it, not the library."""
    for name in ctx.TUNING:
        v = os.environ.get("WSG_TUNE_" + name.upper())
        if v is not None:
            ctx.set_tuning(name, int(v))

def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None, help="GPUs (rank processes); default WORLD_SIZE or 1")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--event-every", type=int, default=4,
                    help="timed steps bracket the streaming kernel with a HIP event pair in one step of "
                         "this many (an event pair costs ~12 us of queue time: tools/ubench_graph.hip)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="north",
                    help="per-GPU workload: north (1M x 4 KiB TEXT), 1 (configs[1]), 3 (configs[3] shard, 8M x 4 KiB)")
    ap.add_argument("--frames", type=int, default=None, help="frames per GPU (overrides --config)")
    ap.add_argument("--payload", type=int, default=None)
    ap.add_argument("--sessions", type=int, default=None, help="sessions per GPU")
    ap.add_argument("--binary", action="store_true", help="BINARY frames (unmask only, no UTF-8 work)")
    ap.add_argument("--no-validate", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything beside the headline: the per-kernel "
                         "breakdown, the copy ceiling, the validator stage, the host->device->host lines, the "
                         "secondary configs and the CPU baselines (the options below that trim them apply here)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step's decode left in the caller's buffers as DIR/<name>.npy "
                         "(dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    ap.add_argument("--e2e", action="store_true",
                    help="also time the pinned host->device->host paths (on by default at N=1 with the extra lines)")
    ap.add_argument("--no-e2e", action="store_true", help="skip the host->device->host lines")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the secondary BASELINE configs (measured at N=1 only)")
    ap.add_argument("--extra-steps", type=int, default=10)
    ap.add_argument("--inflate-only", action="store_true", help="only the permessage-deflate inflate line")
    ap.add_argument("--handshake-only", action="store_true", help="only the server handshake line")
    ap.add_argument("--inflate-sessions", type=int, nargs="+", default=[8192])
    ap.add_argument("--only", default=None,
                    help="print only one secondary line: configs1|configs2|configs3|encode|validator|inflate|deflate|"
                         "handshake|hs_client")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    for k in ("frames", "payload", "sessions"):
        if getattr(args, k) is None:
            setattr(args, k, cfg[k])
    args.binary = args.binary or cfg["binary"]
    return args


def child_line(line: str, extra_steps: int = 3, timeout: int = 300) -> dict:
    """One secondary line measured by `python bench.py --only <line>` in a child process
    (started, not exec'd: this process has the GPU) — its JSON line, marked as such."""
    cmd = [sys.executable, os.path.abspath(__file__), "--only", line, "--no-cpu-baseline",
           "--extra-steps", str(extra_steps)]
    try:
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"error": f"timed out after {timeout} s", "cmd": " ".join(cmd[1:])}
    rows = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not rows:
        return {"error": f"exit {p.returncode}: {p.stderr.strip()[-300:]}", "cmd": " ".join(cmd[1:])}
    out = json.loads(rows[-1])
    out["process"] = f"own process: python bench.py --only {line}"
    return out


def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_or_check_world(args) -> int:
    """The N of --gpus N.  Without a torch.distributed environment and N > 1, start
    the N rank processes (one per GPU) as children of this process and exit with
    their status: nothing here has touched a GPU yet.  Under a launcher, --gpus must
    match WORLD_SIZE, so a line never reports fewer GPUs than were asked for."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None:
        n = 1 if args.gpus is None else args.gpus
        if n > 1:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
                   "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", os.path.abspath(__file__),
                   *sys.argv[1:]]
            sys.exit(subprocess.call(cmd))
        return 1
    world = int(env_world)
    if args.gpus is not None and args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} (one rank process per GPU)")
    return world


def cpu_quota() -> float | None:
    """CPUs this process's cgroup may use (cgroup v2 cpu.max quota / period), if capped."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, p = fh.read().split()[:2]
        return None if q == "max" else int(q) / int(p)
    except (OSError, ValueError):
        return None


def cpu_threads() -> tuple[int, str]:
    """Host threads for the N-thread CPU baseline: every CPU this process may run on
    (sched_getaffinity), except that on the GPU box the harness allots one GPU's job a
    CPU share (OMP_NUM_THREADS / the cgroup quota, 16) and asks worker pools to stay
    within it — the affinity mask there lists the whole shared machine.  Both counts
    are stated beside the figure."""
    aff = len(os.sched_getaffinity(0))
    quota = cpu_quota()
    omp = os.environ.get("OMP_NUM_THREADS")
    share = int(omp) if omp and omp.isdigit() and int(omp) > 0 else None
    if quota is not None:
        share = min(share or aff, max(1, int(quota)))
    if share and share < aff:
        return share, (f"{share} = the job's CPU share (OMP_NUM_THREADS={omp}, cgroup quota "
                       f"{'none' if quota is None else f'{quota:g} CPUs'}); sched_getaffinity lists {aff} CPUs "
                       f"of the shared host")
    return aff, f"sched_getaffinity={aff} (every CPU this process may use)"


def config0_line():
    """configs[0]: the reference's loopback echo (snf4j SelectorLoop, Java) on the CPU.
    Needs a JDK and the snf4j jars on the box; reported, never substituted."""
    java = shutil.which("java")
    return {"config": "configs[0]: snf4j-websocket loopback echo over 127.0.0.1, 1 session, 4 KiB masked binary "
                      "frames (CPU reference codec, no GPU)",
            "status": ("not runnable (java found at %s, but the snf4j jars do not travel to the box)" % java
                       if java else "not runnable (no JDK on the box: `java` not on PATH)"),
            "value": None}


def cpu_baseline(args, seconds):
    """The oracle (single-threaded C restatement of the reference codec) on a bounded
    sample of the same workload; test infrastructure, timed beside the GPU."""
    import numpy as np
    from oracle import pyoracle
    pyoracle.build()
    n = min(args.frames, 16384)
    fps = max(1, args.frames // args.sessions)
    wire, off, sf = pyoracle.synth_uniform(1234, n, args.payload, min(fps, n), opcode=2 if args.binary else 1,
                                           masked=True, text=not args.binary)
    n_s = len(sf) - 1
    done, t = 0, 0.0
    while t < seconds:
        b = pyoracle.Batch(False, False, 65536, not args.no_validate, n_s)
        t0 = time.perf_counter()
        _, _, res = b.decode(wire, off, sf)
        t += time.perf_counter() - t0
        assert int(res["error"].max()) == 0
        done += 1
    gib = done * int(off[-1]) / t / 2**30
    return {"value": round(gib, 4), "unit": "GiB/s", "cores": 1, "kind": "port",
            "sample": f"{n} frames x {args.payload} B ({int(off[-1]) / 1e6:.1f} MB wire) decoded {done}x "
                      f"in {t:.1f} s by the C restatement of FrameDecoder+FrameUtf8Validator (oracle/, 1 thread; "
                      f"no JDK on the box, the Java reference is not runnable)"}


def cpu_baseline_mt(args, seconds):
    """The same C restatement on N host threads (cpu_threads()), one Batch (own
    sessions) per thread: the N-thread figure SURVEY.md §8(d) asks for beside the
    1-thread one.  ctypes releases the GIL around each oracle call, so the threads
    decode in parallel."""
    import threading
    from oracle import pyoracle
    pyoracle.build()
    threads, how = cpu_threads()
    n = min(args.frames, 16384)
    fps = max(1, args.frames // args.sessions)
    wire, off, sf = pyoracle.synth_uniform(1234, n, args.payload, min(fps, n), opcode=2 if args.binary else 1,
                                           masked=True, text=not args.binary)
    n_s = len(sf) - 1
    counts = [0] * threads
    stop = time.perf_counter() + seconds

    def work(i):
        b = pyoracle.Batch(False, False, 65536, not args.no_validate, n_s)
        while time.perf_counter() < stop:
            b.decode(wire, off, sf)
            counts[i] += 1

    ts = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    el = time.perf_counter() - t0
    gib = sum(counts) * int(off[-1]) / el / 2**30
    return {"value": round(gib, 4), "unit": "GiB/s", "cores": threads, "kind": "port", "cores_from": how,
            "sample": f"{threads} threads, each decoding {n} frames x {args.payload} B repeatedly for {el:.1f} s "
                      f"({sum(counts)} batches) with the C restatement (oracle/)"}


def main():
    args = parse()
    EVENT_EVERY[0] = max(1, args.event_every)
    world = launch_or_check_world(args)  # (may start the rank processes and exit)
    import numpy as np
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        # the data path has no collective; gloo carries only the barrier and the timing max
        dist.init_process_group("gloo")
    # WSG_BENCH_ONE_DEVICE=1 puts every rank on device 0: a rehearsal of the N>1
    # code path (barrier, max over ranks) on a 1-GPU box, never a reported number
    one_device = os.environ.get("WSG_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local = 0
    elif local >= torch.cuda.device_count():
        sys.exit(f"bench.py: rank {rank} needs GPU {local}, but {torch.cuda.device_count()} are visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    import snf4j_amd
    from snf4j_amd._lib import RESULT_DTYPE
    from snf4j_amd.shard import rank_seed, time_steps

    stream = torch.cuda.current_stream(dev)
    ctx = snf4j_amd.Context(local, stream=stream)
    apply_tuning(ctx)
    if args.only:
        print(json.dumps(EXTRA_LINES[args.only](ctx, dev, args.extra_steps, 2)), flush=True)
        ctx.close()
        return
    if args.handshake_only:
        print(json.dumps(handshake_line(ctx, dev, args.extra_steps, 2)), flush=True)
        return
    if args.inflate_only:
        for n_s in args.inflate_sessions:
            print(json.dumps(inflate_line(ctx, dev, args.extra_steps, 2, n_s=n_s, cpu_seconds=0.2)), flush=True)
        ctx.close()
        return
    F, P = args.frames, args.payload
    flen = snf4j_amd.encoded_length(P, True)
    fps = max(1, F // args.sessions)
    n_s = (F + fps - 1) // fps
    text = 0 if args.binary else 1
    opcode = 2 if args.binary else 1
    wire = torch.empty(F * flen + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(F + 1, dtype=torch.int64, device=dev)
    sf = torch.empty(n_s + 1, dtype=torch.int32, device=dev)
    # sessions of rank r are global sessions [r*n_s, (r+1)*n_s): shard by session, own seed
    benchsupport.synth_uniform(ctx, rank_seed(0x5EED, rank), F, P, fps, opcode, True, text, wire, off, sf)
    payload_cap = F * flen + 16 * F + 16
    payload = torch.empty(payload_cap, dtype=torch.uint8, device=dev)
    desc = torch.empty(F * 16, dtype=torch.uint8, device=dev)
    res = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)
    state = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    cfg = snf4j_amd.decoder_cfg(False, False, 65536, not args.no_validate)
    ctx.reserve(F, n_s, F * flen)
    wire_bytes = F * flen

    def step():
        ctx.decode_device(cfg, wire, off, sf, state, payload, desc, res, wire_len=wire_bytes)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    r = res.cpu().numpy().view(RESULT_DTYPE)
    assert int(r["error"].max()) == 0 and int(r["n_delivered"].sum()) == F, "decode of the synthetic batch failed"

    # timed region: events around the streaming kernel only (its roofline figure)
    ctx.reset_timing()
    ctx.set_timing("hot")
    ctx.set_timing_every(EVENT_EVERY[0])
    elapsed = time_steps(step, args.steps, sync=lambda: torch.cuda.synchronize(dev), dist=dist)
    ctx.set_timing(False)
    ctx.set_timing_every(1)
    timing = ctx.timing()
    if args.dump_outputs:  # (before any further step() and before copy_ceiling: both overwrite the buffers)
        dump_outputs(args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, f"rank{rank}"),
                     payload, desc, res, state, F)
    full = args.full  # everything beside the headline figure
    pipe = pipeline_breakdown(ctx, step, dev) if full else None
    validator = None  # (before copy_ceiling, which overwrites the payload buffer)
    if full and world == 1 and not args.no_extras and not args.binary:
        validator = validator_line(ctx, dev, desc, sf, payload, n_s, F, P, args.extra_steps)

    # dominant kernel: k_piecesN reads each frame's payload bytes off the wire and writes them unmasked
    unmask_ms, unmask_n = timing["k_piecesN"]
    avg_unmask_s = unmask_ms / 1e3 / max(1, unmask_n)
    alg_bytes = wire_bytes + F * P  # per launch: wire read + payload written
    copy = benchsupport.copy_ceiling(ctx, wire, payload, wire_bytes) if full else None
    achieved = alg_bytes / avg_unmask_s / 1e9
    # HBM bytes per launch from the PMC counters: PMC cannot run in the same process as
    # the timed region (separate rocprofv3 --pmc passes, MI355X_MICROARCH.md), so this is
    # the committed measurement of the same kernel on the same workload, labelled with
    # its file (traffic_source); null when none exists for this workload
    traffic = traffic_source = None
    if full and os.path.exists(args.pmc_json):
        try:
            with open(args.pmc_json) as fh:
                pmc = json.load(fh)
            key = f"{'binary' if args.binary else 'text'}_{F}x{P}"
            traffic = pmc.get(key, {}).get("hbm_bytes_per_launch")
            if traffic is not None:
                traffic_source = (os.path.relpath(args.pmc_json, ROOT) + f" [{key}] <- " +
                                  pmc[key].get("source", "") + " (a separate PMC run, not this process)")
        except Exception:
            traffic = traffic_source = None

    e2e = None
    if full and (args.e2e or (world == 1 and not args.no_extras)) and not args.no_e2e:
        e2e = e2e_rate(ctx, cfg, wire, off, sf, n_s, wire_bytes, F, dev)

    extras = None
    if full and world == 1 and not args.no_extras:
        del wire, payload, desc, res, state, off, sf
        torch.cuda.empty_cache()
        # the pinned buffers of the lines above (≈ 13 GB, held by torch's pinned-memory
        # cache) go back before the host-to-host batcher lines
        gc.collect()
        if hasattr(torch._C, "_host_emptyCache"):
            torch._C._host_emptyCache()
        if e2e is not None:
            # Each host-to-host batcher line in a process of its own (`python bench.py
            # --only <line>`, started as a child; this one waits): a batcher's streams share
            # the process's hardware queues with every stream created before them, and in
            # this process, after the lines above, that alone moved the encode batcher
            # 27-40 GiB/s and the stage line 17-22 — a server process
            # runs its loops' batchers, not a benchmark's other lines.  Two untimed passes
            # each (one was not enough: a round-5 probe, profiles/r05_ab).
            torch.cuda.synchronize()
            for key, line in (("native_batcher_stages", "e2e_stages"),  # batcher -> inflate -> validator
                              # the same sessions streaming 4x longer: the burst line's pipeline
                              # fill and drain amortised over ~20 flushes
                              ("native_batcher_stages_steady", "e2e_stages_steady"),
                              ("native_encode_batcher", "e2e_encode"), ("native_batcher_aggregate", "e2e_aggregate"),
                              # 1, 2 and 4 loops of one process on one device (the JVM's shape)
                              ("native_batcher_stages_multi_loop", "e2e_stages_multi")):
                e2e[key] = child_line(line)
        extras = [config0_line()] + measure_extras(ctx, dev, args)

    # the CPU baseline runs after every timed region, on rank 0 only (at N > 1 the
    # other ranks wait for it at the closing barrier)
    cpu = cpu_mt = None
    if full and rank == 0 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args, args.cpu_seconds)
        cpu_mt = cpu_baseline_mt(args, 5.0)

    if rank == 0:
        total_wire = wire_bytes * world
        value = total_wire * args.steps / elapsed / 2**30
        ms_step = elapsed / args.steps * 1e3
        out = {
            "metric": METRIC,
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {
                "baseline_config": {"north": "north star (1 GPU)", "1": "configs[1]",
                                    "3": "configs[3] (per-GPU shard of 64M x 4 KiB over 8 GPUs)"}[args.config],
                "workload": (f"{F} x {P} B masked {'BINARY' if args.binary else 'TEXT'} frames per GPU, "
                             f"{n_s} sessions per GPU, unmask{'' if args.binary or args.no_validate else ' + UTF-8 validation'}"
                             f", server-side decode (FrameDecoder+FrameUtf8Validator)"),
                "frames_per_gpu": F,
                "payload_bytes": P,
                "wire_bytes_per_gpu": wire_bytes,
                "sessions_per_gpu": n_s,
                "parallelism": f"sessions sharded over {world} GPU(s), one process per GPU, no data-path collective",
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "k_piecesN",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "traffic_source": traffic_source,
                "alg_bytes_per_launch": alg_bytes,
                "avg_launch_ms": round(avg_unmask_s * 1e3, 4),
                "launches_timed": int(unmask_n), "event_every": EVENT_EVERY[0],
                # the north star's "HBM read-bandwidth fraction": wire bytes read / time / 8 TB/s,
                # over the streaming kernel and over the whole step
                "read_frac": round(wire_bytes / avg_unmask_s / 1e9 / HBM_PEAK_GBS, 4),
                "read_frac_step": round(wire_bytes / (ms_step / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
            },
            "full": full,
        }
        if full:
            out["roofline"].update({"copy_ceiling_GBs": round(copy, 1),
                                    "frac_of_copy_ceiling": round(achieved / copy, 4)})
            out.update({"pipeline_ms": pipe, "cpu_baseline": cpu, "cpu_baseline_threads": cpu_mt})
        # NOT measured by this run: the same kernel's mean launch in the committed rocprofv3
        # profile of this workload (another process, maybe another build or box), kept
        # apart from the measured roofline block as a cross-reference
        prof_ms, prof_src = (None, None) if not full else \
            profiled_launch("north" if args.config == "north" and not args.binary else
                            {"1": "configs1", "3": "configs3"}.get(args.config, "north"),
                            "k_piecesN<1, 1, 2")  # (rocprof prints the defaulted template arguments too)
        if prof_ms and F == 1 << 20 and P == 4096 and not args.binary:
            pf = alg_bytes / (prof_ms / 1e3) / 1e9 / HBM_PEAK_GBS
            out["reference_profile"] = {"source": prof_src, "launch_ms": round(prof_ms, 4), "frac": round(pf, 4),
                                        "note": "committed profile, not this run (compare with roofline.frac)"}
        if e2e:
            out["e2e_pinned"] = e2e
        if validator:
            out["validator_stage"] = validator
        if extras:
            out["configs_measured"] = extras
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist:
        dist.barrier()  # (the other ranks wait here for rank 0's CPU baseline)
        dist.destroy_process_group()


DUMP_FRAMES = 1 << 20         # descriptors dumped (all of them up to this many frames)
DUMP_PAYLOAD_FRAMES = 1024    # frames whose payload bytes are dumped
DUMP_PAYLOAD_BYTES = 8 << 20  # ... and at most this many bytes of them


def dump_outputs(dirname, payload, desc, res, state, F):
    """--dump-outputs: what decode_device left in the caller's buffers after the last timed
    step, as float .npy files (every value is an integer a float64 / float32 holds exactly):
      frames.npy           the frames whose descriptors are dumped: all up to DUMP_FRAMES, a
                           fixed seeded sample of a larger batch
      desc_<field>.npy     FrameDesc fields of those frames
      result_<field>.npy   SessionResult fields of every session
      state.npy            SessionState bytes of every session, [sessions, 8]
      payload_frames.npy   the frames whose payloads are dumped (a fixed seeded sample)
      payload_bytes.npy    their unmasked payload bytes, concatenated in that order
    About 55 MB at the default workload.  Samples depend on F alone."""
    import numpy as np
    import torch
    from snf4j_amd._lib import DESC_DTYPE, RESULT_DTYPE
    os.makedirs(dirname, exist_ok=True)

    def save(name, a, dt):
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a, dtype=dt))

    rng = np.random.default_rng(0xD0C5)
    frames = np.arange(F) if F <= DUMP_FRAMES else np.sort(rng.choice(F, DUMP_FRAMES, replace=False))
    d = desc.cpu().numpy().view(DESC_DTYPE)[frames]
    save("frames", frames, np.float64)
    for name in ("payload_off", "payload_len"):
        save("desc_" + name, d[name], np.float64)
    for name in ("opcode", "flags", "status"):
        save("desc_" + name, d[name], np.float32)
    r = res.cpu().numpy().view(RESULT_DTYPE)
    for name in RESULT_DTYPE.names:
        save("result_" + name, r[name], np.float64)
    save("state", state.cpu().numpy().reshape(-1, 8), np.float32)
    pick = np.sort(rng.choice(len(frames), min(len(frames), DUMP_PAYLOAD_FRAMES), replace=False))
    lens = d["payload_len"][pick].astype(np.int64)
    pick = pick[np.cumsum(lens) <= DUMP_PAYLOAD_BYTES]
    offs, lens = d["payload_off"][pick].astype(np.int64), d["payload_len"][pick].astype(np.int64)
    # gather the picked frames' byte ranges on the device: one index per dumped byte
    start = np.repeat(offs - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    got = payload[torch.from_numpy(start).to(payload.device)].cpu().numpy()
    save("payload_frames", frames[pick], np.float64)
    save("payload_bytes", got, np.float32)


def profiled_launch(line: str, kernel_prefix: str):
    """The committed rocprofv3 --kernel-trace --stats summary of this bench line
    (profiles/<round>_<line>_kernel_stats.csv, the newest round): the kernel's mean
    launch duration (ms) and the file, so the line can print the roofline fraction the
    profile gives beside the one its own HIP events give (a box-to-box delta otherwise)."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{line}_kernel_stats.csv")))
    if not files:
        return None, None
    with open(files[-1]) as fh:
        for row in csv.DictReader(fh):
            if kernel_prefix in row["Name"]:
                return float(row["AverageNs"]) / 1e6, os.path.relpath(files[-1], ROOT)
    return None, None


def validator_line(ctx, dev, desc, sf, payload, n_s, F, P, steps):
    """The standalone "ws-utf8-validator" stage (wsg_validate_batch_device: the split-off
    validation a permessage-deflate session needs after inflate) over the decoded
    headline batch's plain payloads: read-only streaming, roofline = payload bytes read."""
    import torch
    from snf4j_amd._lib import RESULT_DTYPE
    vstate = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    vres = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)

    def step():
        vstate.zero_()
        ctx.validate_device(desc, sf, payload, vstate, vres, n_frames=F)

    step()
    torch.cuda.synchronize(dev)
    r = vres.cpu().numpy().view(RESULT_DTYPE)
    assert int(r["error"].max()) == 0 and int(r["n_delivered"].sum()) == F
    el, kms, pipe = _timed(ctx, step, steps, 2, dev, "k_piecesN")
    alg = F * P
    ach = alg / (kms / 1e3) / 1e9
    return {"config": f"FrameUtf8Validator stage alone over {F} x {P} B plain TEXT payloads (decoded headline batch)",
            "value": round(alg * steps / el / 2**30, 3), "unit": "GiB/s (payload)",
            "ms_per_step": round(el / steps * 1e3, 4),
            "roofline": {"kernel": "k_piecesN (validate only, no stores)", "achieved": round(ach, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                         "alg_bytes_per_launch": alg, "avg_launch_ms": round(kms, 4)},
            "pipeline_ms": pipe}


EVENT_EVERY = [4]  # set from --event-every in main()


def pipeline_breakdown(ctx, step, dev, steps=5):
    """Per-kernel averages (ms) from a separate, untimed pass with an event pair
    around every kernel (diagnostic: the pairs themselves add queue time)."""
    import torch
    torch.cuda.synchronize(dev)
    ctx.reset_timing()
    ctx.set_timing(True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    ctx.set_timing(False)
    tm = ctx.timing()
    ctx.reset_timing()
    return {k: round(v[0] / max(1, v[1]), 4) for k, v in tm.items() if v[1]}


def _timed(ctx, step, steps, warmup, dev, kernel):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    ctx.reset_timing()
    ctx.set_timing("hot")
    ctx.set_timing_every(EVENT_EVERY[0])
    from snf4j_amd.shard import time_steps
    el = time_steps(step, steps, sync=lambda: torch.cuda.synchronize(dev))
    ctx.set_timing(False)
    ctx.set_timing_every(1)
    tm = ctx.timing()
    # a list of kernels: the sum of their average durations (a pipeline of launches per step)
    kms = sum(tm[k][0] / max(1, tm[k][1]) for k in (kernel if isinstance(kernel, (list, tuple)) else [kernel]))
    return el, kms, pipeline_breakdown(ctx, step, dev)


def _aggregate_line(ctx, dev, payload, desc, res, sf, n, n_s, steps, warmup, max_len=1 << 20):
    """FrameAggregator (wsg_aggregate_batch_device) over the decoded batch: every
    fragmented message's bytes gathered into one contiguous range.  k_agg_gather's
    algorithmic bytes = member bytes read + written."""
    import torch
    from snf4j_amd._lib import RESULT_DTYPE
    cap = payload.numel()
    agg_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    out_desc = torch.empty((n + n_s) * 16, dtype=torch.uint8, device=dev)
    out_res = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)
    astate = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def step():
        astate.zero_()
        ctx.aggregate_device(max_len, desc, sf, res, payload, astate, agg_out, out_desc, out_res, total, n_frames=n)

    step()
    torch.cuda.synchronize(dev)
    member = int(total.item())
    r = out_res.cpu().numpy().view(RESULT_DTYPE)
    assert int((r["error"] != 0).sum()) == 0
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, "k_agg_gather")
    ach = 2 * member / (kms / 1e3) / 1e9
    return {"config": "FrameAggregator over the decoded configs[2] batch (maxAggregatedLength 1 MiB)",
            "value": round(member * steps / el / 2**30, 3), "unit": "GiB/s (aggregated message bytes)",
            "ms_per_step": round(el / steps * 1e3, 4), "member_bytes": member,
            "output_frames": int(r["n_delivered"].sum()),
            "roofline": {"kernel": "k_agg_gather", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": 2 * member,
                         "avg_launch_ms": round(kms, 4)},
            "pipeline_ms": {k: v for k, v in pipe.items() if k.startswith("k_agg")}}


def inflate_line(ctx, dev, steps, warmup, n_s=8192, msgs=16, msg_bytes=4096, cpu_seconds=3.0):
    """PerMessageDeflateDecoder (wsg_inflate_batch_device) over a device-resident batch of
    compressed TEXT messages, context takeover.  Serial Huffman/LZ77
    per session: the bound is per-workgroup decode latency, not HBM; the roofline figure
    is reported against HBM for scale only.  cpu_baseline: zlib (the engine of
    java.util.zip.Inflater that DeflateDecoder drives) on one host core."""
    import zlib
    import numpy as np
    import torch
    from snf4j_amd._lib import DESC_DTYPE, RESULT_DTYPE
    from benchsupport.synth import deflate_batch
    desc_h, sf_h, pl_h, plain = deflate_batch(0x1F1A, n_s, msgs, msg_bytes)
    n = len(desc_h)
    cap = msgs * msg_bytes
    desc = torch.from_numpy(desc_h.view(np.uint8).copy()).to(dev)
    sf = torch.from_numpy(sf_h.view(np.int32).copy()).to(dev)
    payload = torch.from_numpy(pl_h.copy()).to(dev)
    state = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    window = torch.empty(n_s * 32768, dtype=torch.uint8, device=dev)
    out = torch.empty(n_s * cap, dtype=torch.uint8, device=dev)
    out_off = torch.arange(n_s + 1, dtype=torch.int64, device=dev) * cap
    odesc = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    ores = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)
    rf = torch.empty(n_s, dtype=torch.int32, device=dev)

    def step():
        state.zero_()  # every step inflates the same streams from fresh decoders
        ctx.inflate_device(False, desc, sf, payload, state, window, out, out_off, odesc, ores, rf, n_frames=n)

    step()
    torch.cuda.synchronize(dev)
    r = ores.cpu().numpy().view(RESULT_DTYPE)
    assert int(r["error"].max()) == 0 and int(r["n_delivered"].sum()) == n
    od = odesc.cpu().numpy().view(DESC_DTYPE)
    assert int(od["payload_len"].astype(np.int64).sum()) == plain
    # spot check: sessions 0 and n_s-1 against zlib
    oh = None
    for s in (0, n_s - 1):
        d = zlib.decompressobj(-15)
        k0 = int(sf_h[s])
        for k in range(k0, k0 + msgs):
            o, ln = int(desc_h[k]["payload_off"]), int(desc_h[k]["payload_len"])
            exp = d.decompress(pl_h[o:o + ln].tobytes() + b"\x00\x00\xff\xff")
            go, gl = int(od[k]["payload_off"]), int(od[k]["payload_len"])
            if oh is None:
                oh = out.cpu().numpy()
            assert oh[go:go + gl].tobytes() == exp, ("inflate mismatch", s, k)
    del oh
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, ["k_infl_tok", "k_infl_fast", "k_inflate"])
    comp = int(pl_h.size) - 16
    alg = comp + plain
    ach = alg / (kms / 1e3) / 1e9
    # CPU: zlib over the first sessions' streams, one thread
    done, t = 0, 0.0
    while t < cpu_seconds:
        s = done % 64
        k0 = int(sf_h[s])
        t0 = time.perf_counter()
        d = zlib.decompressobj(-15)
        for k in range(k0, k0 + msgs):
            o, ln = int(desc_h[k]["payload_off"]), int(desc_h[k]["payload_len"])
            d.decompress(pl_h[o:o + ln].tobytes() + b"\x00\x00\xff\xff")
        t += time.perf_counter() - t0
        done += 1
    cpu = done * msgs * msg_bytes / t / 2**30
    return {"config": f"permessage-deflate inflate: {n_s} sessions x {msgs} TEXT messages x {msg_bytes} B, "
                      f"context takeover, level 6 (compressed {comp / 1e6:.0f} MB -> {plain / 1e6:.0f} MB)",
            "value": round(plain * steps / el / 2**30, 3), "unit": "GiB/s (inflated bytes)",
            "ms_per_step": round(el / steps * 1e3, 4),
            "roofline": {"kernel": "k_infl_tok + k_infl_fast + k_inflate (the inflate launches of a step)",
                         "bound": "per-lane Huffman decode latency (k_infl_tok), not hbm",
                         "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "cpu_baseline": {"value": round(cpu, 4), "unit": "GiB/s (inflated bytes)", "cores": 1,
                             "kind": "zlib",
                             "sample": f"{done} session streams ({msgs} x {msg_bytes} B) inflated by zlib "
                                       f"(java.util.zip.Inflater's engine) in {t:.1f} s, 1 thread"},
            "pipeline_ms": pipe}


def deflate_line(ctx, dev, steps, warmup, n_s=8192, msgs=16, msg_bytes=4096, level=6, cpu_seconds=3.0):
    """PerMessageDeflateEncoder (wsg_deflate_batch_device) over a device-resident batch of
    TEXT messages, context takeover, level 6 (the compressing side):
    every byte identical to zlib's (java.util.zip.Deflater's engine).  A step compresses
    every session's messages from a new deflater.  The bound is the per-position match
    search and the per-frame lazy parse (latency and issue), not HBM; the roofline figure
    is reported against HBM for scale.  cpu_baseline: zlib level 6 driven as ZlibEncoder
    drives Deflater (oracle/deflate_ref.c) on 1 host thread and on the job's threads."""
    import threading
    import numpy as np
    import torch
    from benchsupport.synth import deflate_plain
    from oracle import deflateref
    from snf4j_amd._lib import DESC_DTYPE
    from snf4j_amd.context import DEFLATE_SESSION_BYTES
    bodies = deflate_plain(0xDEF1, n_s, msgs, msg_bytes)
    n = n_s * msgs
    lens = np.array([len(m) for ms in bodies for m in ms], dtype=np.uint64)
    desc_h = np.zeros(n, dtype=DESC_DTYPE)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(lens)[:-1]
    desc_h["payload_off"], desc_h["payload_len"], desc_h["opcode"], desc_h["flags"] = off, lens, 1, 0x80
    plain = int(lens.sum())
    pl_h = np.frombuffer(b"".join(m for ms in bodies for m in ms) + bytes(16), dtype=np.uint8)
    sf_h = (np.arange(n_s + 1) * msgs).astype(np.uint32)
    desc = torch.from_numpy(desc_h.view(np.uint8).copy()).to(dev)
    sf = torch.from_numpy(sf_h.view(np.int32).copy()).to(dev)
    payload = torch.from_numpy(pl_h.copy()).to(dev)
    state = torch.zeros(n_s * 16, dtype=torch.uint8, device=dev)
    smem = torch.empty(n_s * DEFLATE_SESSION_BYTES, dtype=torch.uint8, device=dev)
    bound = int(((lens + ((lens + 7) >> 3) + ((lens + 63) >> 6) + 15 + 15) >> 4 << 4).sum())
    out = torch.empty(bound + 16, dtype=torch.uint8, device=dev)
    odesc = torch.empty(n * 16, dtype=torch.uint8, device=dev)

    def step():
        state.zero_()   # new deflaters: every step compresses the same streams from the start
        ctx.deflate_device(level, False, desc, sf, payload, state, smem, out, odesc, n_frames=n)

    step()
    torch.cuda.synchronize(dev)
    od = odesc.cpu().numpy().view(DESC_DTYPE)
    comp = int(od["payload_len"].astype(np.int64).sum())
    oh = None
    for s in (0, n_s - 1):   # spot check against zlib driven as Deflater is
        ref = deflateref.encode_frames([(1, True, 0, m) for m in bodies[s]], level, False)
        if oh is None:
            oh = out.cpu().numpy()
        for i, k in enumerate(range(s * msgs, (s + 1) * msgs)):
            o, ln = int(od[k]["payload_off"]), int(od[k]["payload_len"])
            assert oh[o:o + ln].tobytes() == ref[i][3] and int(od[k]["flags"]) == 0x80 | 0x40 | 0x02, \
                ("deflate mismatch", s, i)
    del oh
    kernels = ["k_defl_prep", "k_defl_links", "k_defl_match_lds", "k_defl_match", "k_defl_parse"]
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, kernels)
    alg = plain + comp
    ach = alg / (kms / 1e3) / 1e9
    # CPU: zlib level 6 over whole session streams (16 x 4 KiB each), 1 thread then N threads
    slens = np.array([len(m) for m in bodies[0]], dtype=np.uint32)

    def sess_data(s):
        return np.frombuffer(b"".join(bodies[s]), dtype=np.uint8)

    data = [sess_data(s) for s in range(64)]
    done, t = 0, 0.0
    while t < cpu_seconds:
        t0 = time.perf_counter()
        deflateref.stream_bytes(level, slens, data[done % 64])
        t += time.perf_counter() - t0
        done += 1
    cpu1 = done * int(slens.sum()) / t / 2**30
    threads, how = cpu_threads()
    counts = [0] * threads
    stop = time.perf_counter() + cpu_seconds

    def work(i):
        j = i
        while time.perf_counter() < stop:
            deflateref.stream_bytes(level, slens, data[j % 64])
            counts[i] += 1
            j += threads

    ts = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
    t0 = time.perf_counter()
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    elt = time.perf_counter() - t0
    cpun = sum(counts) * int(slens.sum()) / elt / 2**30
    return {"config": f"permessage-deflate compress: {n_s} sessions x {msgs} TEXT messages x {msg_bytes} B, "
                      f"context takeover, level {level} ({plain / 1e6:.0f} MB -> {comp / 1e6:.0f} MB, "
                      f"byte-identical to zlib)",
            "value": round(plain * steps / el / 2**30, 3), "unit": "GiB/s (uncompressed bytes)",
            "ms_per_step": round(el / steps * 1e3, 4),
            "roofline": {"kernel": "k_defl_prep + k_defl_links + k_defl_match_lds + k_defl_match + k_defl_parse (the compress launches of a step)",
                         "bound": "per-position hash-chain match search and per-frame lazy parse (latency, issue), "
                                  "not hbm",
                         "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "cpu_baseline": {"value": round(cpu1, 4), "unit": "GiB/s (uncompressed bytes)", "cores": 1,
                             "kind": "zlib",
                             "sample": f"{done} session streams ({msgs} x {msg_bytes} B) deflated at level {level} "
                                       f"by zlib driven as ZlibEncoder drives java.util.zip.Deflater "
                                       f"(oracle/deflate_ref.c) in {t:.1f} s, 1 thread"},
            "cpu_baseline_threads": {"value": round(cpun, 4), "unit": "GiB/s (uncompressed bytes)",
                                     "cores": threads, "kind": "zlib", "cores_from": how,
                                     "sample": f"{sum(counts)} session streams on {threads} threads in {elt:.1f} s"},
            "pipeline_ms": pipe}


def _decode_line(ctx, dev, name, wire, wl, off, sf, n, n_s, payload_bytes, steps, warmup, expect_errors=None,
                 aggregate=False):
    """Decode GiB/s (wire) + k_piecesN roofline of one device-resident batch."""
    import numpy as np
    import torch
    from snf4j_amd import decoder_cfg
    from snf4j_amd._lib import RESULT_DTYPE, lib
    cap = int(lib.wsg_decode_payload_bound(wl, n))
    payload = torch.empty(cap, dtype=torch.uint8, device=dev)
    desc = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    res = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)
    state = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    cfg = decoder_cfg(False, False, 65536, True)
    ctx.reserve(n, n_s, wl)

    def step():
        state.zero_()  # every step decodes the same batch from a fresh session state
        ctx.decode_device(cfg, wire, off, sf, state, payload, desc, res, wire_len=wl)

    step()
    torch.cuda.synchronize(dev)
    r = res.cpu().numpy().view(RESULT_DTYPE)
    n_err = int((r["error"] != 0).sum())
    if expect_errors is not None:
        assert n_err == expect_errors, (name, n_err, expect_errors)
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, "k_piecesN")
    alg = wl + payload_bytes
    ach = alg / (kms / 1e3) / 1e9
    agg = _aggregate_line(ctx, dev, payload, desc, res, sf, n, n_s, steps, warmup) if aggregate else None
    pipe = {k: v for k, v in pipe.items() if not k.startswith("k_agg")}
    return {"config": name, "value": round(wl * steps / el / 2**30, 3), "unit": "GiB/s (wire)",
            "ms_per_step": round(el / steps * 1e3, 4), "frames": n, "sessions": n_s, "wire_bytes": wl,
            "sessions_with_error": n_err,
            "roofline": {"kernel": "k_piecesN", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "pipeline_ms": pipe, **({"aggregate": agg} if agg else {})}


def _hs_port_baselines(buf, n, L, keys=None, seconds=3.0):
    """The compiled handshake port (oracle/handshake_port.c: parse + SHA-1 + Base64 a
    request, kind "port") over a bounded sample of the line's requests (or responses), on
    one host core and on the job's cores (cpu_threads)."""
    import numpy as np
    from oracle import handshake_port as HP
    m = min(n, 65536)
    flat = np.ascontiguousarray(buf[:m]).reshape(-1)
    off = (np.arange(m + 1, dtype=np.uint64) * L)
    k = np.ascontiguousarray(keys[:m]).reshape(-1) if keys is not None else None
    what = "responses validated" if keys is not None else "requests accepted"
    r1, d1 = HP.rate(flat, off, k, 1, seconds)
    threads, how = cpu_threads()
    rn, dn = HP.rate(flat, off, k, threads, max(1.0, seconds / 2))
    one = {"value": round(r1 / 1e6, 4), "unit": "M handshakes/s", "cores": 1, "kind": "port",
           "sample": f"{d1} {what} by the compiled C port (oracle/handshake_port.c: HttpUtils framing, "
                     f"HandshakeFactory.parse, Handshaker checks, SHA-1 + Base64, response format) over {m} "
                     f"distinct {L}-B buffers, 1 thread; no JDK on the box"}
    mt = {"value": round(rn / 1e6, 4), "unit": "M handshakes/s", "cores": threads, "kind": "port", "cores_from": how,
          "sample": f"{dn} {what} by the same port on {threads} threads"}
    return one, mt


def handshake_line(ctx, dev, steps, warmup, n=1 << 20, cpu_seconds=2.0):
    """Server opening handshakes (wsg_handshake_accept_batch_device)
    over a device-resident connection storm: n browser-like upgrade requests, random keys.
    One lane per request: the bound is per-lane serial parsing + SHA-1, reported against
    HBM for scale.  cpu_baseline: the compiled C port (oracle/handshake_port.c) on one host
    core, beside it on the job's cores and the Python restatement (oracle/handshake_oracle.py)
    on one core (no JDK on the box)."""
    import base64
    import numpy as np
    import torch
    from oracle import handshake_oracle as H
    from snf4j_amd._lib import HS_RESP_STRIDE, HS_RESULT_DTYPE, HsConfig
    tmpl = H.request("/chat?room=lobby", [
        ("Host", "ws.example.com:8080"), ("Connection", "Upgrade"), ("Pragma", "no-cache"),
        ("Cache-Control", "no-cache"), ("User-Agent", "Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36"),
        ("Upgrade", "websocket"), ("Origin", "https://example.com"), ("Sec-WebSocket-Version", "13"),
        ("Accept-Encoding", "gzip, deflate, br"), ("Accept-Language", "en-US,en;q=0.9"),
        ("Sec-WebSocket-Key", "A" * 24)])
    L = len(tmpl)
    kpos = tmpl.index(b"A" * 24)
    rng = np.random.default_rng(0x4A5)
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    k24 = np.frombuffer(b"".join(base64.b64encode(r.tobytes()) for r in raw), dtype=np.uint8).reshape(n, 24)
    buf = np.tile(np.frombuffer(tmpl, dtype=np.uint8), (n, 1))
    buf[:, kpos:kpos + 24] = k24
    req = torch.from_numpy(buf.reshape(-1)).to(dev)
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    resp = torch.empty(n * HS_RESP_STRIDE, dtype=torch.uint8, device=dev)
    res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    cfg = HsConfig(65536, 0, 0, 0, 0)

    def step():
        ctx.handshake_accept_device(cfg, req, off, resp, res, n=n)

    step()
    torch.cuda.synchronize(dev)
    r = res.cpu().numpy().view(HS_RESULT_DTYPE)
    assert (r["kind"] == H.ACCEPT).all() and (r["http_status"] == 101).all()
    rh = resp.view(n, HS_RESP_STRIDE)
    for i in (0, 1, n // 2, n - 1):  # spot check against the restatement
        exp = H.accept(buf[i].tobytes())["response"]
        assert rh[i, :int(r["resp_len"][i])].cpu().numpy().tobytes() == exp, i
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, "k_hs_accept")
    rl = int(r["resp_len"][0])
    alg = n * (L + 8 + rl + 16)
    ach = alg / (kms / 1e3) / 1e9
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < cpu_seconds:
        H.accept(buf[done % n].tobytes())
        done += 1
    t = time.perf_counter() - t0
    port1, portn = _hs_port_baselines(buf, n, L)
    return {"config": f"server handshake: {n} upgrade requests of {L} B (browser-like, random keys), "
                      "HandshakeDecoder + Handshaker.accept + 101 response with Sec-WebSocket-Accept",
            "value": round(n * steps / el / 1e6, 3), "unit": "M handshakes/s",
            "ms_per_step": round(el / steps * 1e3, 4),
            "roofline": {"kernel": "k_hs_accept", "bound": "per-lane serial parse + SHA-1 (not hbm)",
                         "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "cpu_baseline": port1, "cpu_baseline_threads": portn,
            "cpu_baseline_python": {"value": round(done / t / 1e6, 5), "unit": "M handshakes/s", "cores": 1,
                                    "kind": "port",
                                    "sample": f"{done} requests through the Python restatement "
                                              f"(oracle/handshake_oracle.py) in {t:.1f} s, 1 thread"},
            "pipeline_ms": pipe}


def line_configs1(ctx, dev, K, W):
    """configs[1]: 1 M masked BINARY frames, 1 KiB payload, 256 sessions (unmask only)."""
    import torch
    from snf4j_amd import encoded_length
    F, P, S = 1 << 20, 1024, 256
    flen = encoded_length(P, True)
    wire = torch.empty(F * flen + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(F + 1, dtype=torch.int64, device=dev)
    sf = torch.empty(S + 1, dtype=torch.int32, device=dev)
    benchsupport.synth_uniform(ctx, 0xC0F2, F, P, F // S, 2, True, 0, wire, off, sf)
    return _decode_line(ctx, dev, "configs[1]: 1M x 1 KiB masked BINARY, 256 sessions", wire, F * flen, off, sf,
                        F, S, F * P, K, W, expect_errors=0)


def line_configs3(ctx, dev, K, W):
    """configs[3]'s per-GPU shard on this GPU: 8 M x 4 KiB masked TEXT, 1024 sessions (34.4 GB in +
    34.4 GB out in one batch; `bench.py --gpus N --config 3` is the scaling run)."""
    import torch
    from snf4j_amd import encoded_length
    c3 = CONFIGS["3"]
    F, P, S = c3["frames"], c3["payload"], c3["sessions"]
    flen = encoded_length(P, True)
    wire = torch.empty(F * flen + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(F + 1, dtype=torch.int64, device=dev)
    sf = torch.empty(S + 1, dtype=torch.int32, device=dev)
    benchsupport.synth_uniform(ctx, 0xC0F4, F, P, F // S, 1, True, 1, wire, off, sf)
    return _decode_line(ctx, dev, "configs[3] per-GPU shard: 8M x 4 KiB masked TEXT, 1024 sessions, "
                        "unmask + UTF-8 (1/8 of 64M x 4 KiB)", wire, F * flen, off, sf,
                        F, S, F * P, max(3, K // 2), W, expect_errors=0)


def line_configs2(ctx, dev, K, W, aggregate=True):
    """configs[2]: mixed text+binary 64 B-64 KiB, UTF-8 on, 1 K sessions, >= 4 GiB wire (+ the
    FrameAggregator line over the decoded batch)."""
    import numpy as np
    import torch
    from benchsupport.synth import mixed_plan
    t, offh, sfh, wl, info = mixed_plan(0xC0F3, 1024, 4 << 30)
    tab = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    wire = torch.zeros(wl + 64, dtype=torch.uint8, device=dev)
    benchsupport.synth_frames(ctx, tab, wire)
    del tab
    line = _decode_line(ctx, dev, "configs[2]: mixed TEXT+BINARY 64 B-64 KiB log-uniform, 10% fragmented, "
                        "1% of text messages with invalid UTF-8, 1024 sessions", wire, wl,
                        torch.from_numpy(offh.astype(np.int64)).to(dev), torch.from_numpy(sfh.astype(np.int32)).to(dev),
                        len(t), 1024, info["payload_bytes"], K, W, expect_errors=len(info["bad_sessions"]),
                        aggregate=aggregate)
    line["mix"] = {k: v for k, v in info.items() if k != "bad_sessions"}
    return line


def line_encode(ctx, dev, K, W):
    """configs[4]: client-side encode, 64 messages x 16 MiB in 64 KiB frames (header emit + mask)."""
    import numpy as np
    import torch
    from snf4j_amd import encoded_length
    from snf4j_amd._lib import ENCODE_DTYPE
    M, FR, FP = 64, 256, 65536
    n = M * FR
    payload = torch.randint(0, 256, (M * FR * FP,), dtype=torch.uint8, device=dev)
    fr = np.zeros(n, dtype=ENCODE_DTYPE)
    fr["payload_off"] = np.arange(n, dtype=np.uint64) * FP
    fr["payload_len"] = FP
    j = np.arange(n) % FR
    fr["opcode"] = np.where(j == 0, 2, 0)
    fr["flags"] = np.where(j == FR - 1, 0x80, 0)
    fr["mask"] = np.random.default_rng(5).integers(0, 256, (n, 4), dtype=np.uint8)
    frames = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    sfe = torch.from_numpy((np.arange(M + 1) * FR).astype(np.int32)).to(dev)
    closed = torch.zeros(M, dtype=torch.uint8, device=dev)
    elen = encoded_length(FP, True)
    wire_out = torch.empty(n * elen + 16, dtype=torch.uint8, device=dev)
    wire_off = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def enc():
        ctx.encode_device(True, payload, frames, sfe, closed, wire_out, wire_off)

    enc()
    torch.cuda.synchronize(dev)
    assert int(wire_off[-1].item()) == n * elen
    el, kms, pipe = _timed(ctx, enc, K, W, dev, "k_enc_piecesN")
    alg = M * FR * FP + n * elen
    ach = alg / (kms / 1e3) / 1e9
    return {"config": "configs[4]: client encode, 64 x 16 MiB messages in 64 KiB frames (header + mask)",
            "value": round(n * elen * K / el / 2**30, 3), "unit": "GiB/s (wire out)",
            "ms_per_step": round(el / K * 1e3, 4), "frames": n,
            "roofline": {"kernel": "k_enc_piecesN", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "pipeline_ms": pipe}


def line_validator(ctx, dev, K, W):
    """The FrameUtf8Validator stage alone over the decoded headline batch (bench --only validator)."""
    import torch
    import snf4j_amd
    c = CONFIGS["north"]
    F, P, S = c["frames"], c["payload"], c["sessions"]
    flen = snf4j_amd.encoded_length(P, True)
    wire = torch.empty(F * flen + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(F + 1, dtype=torch.int64, device=dev)
    sf = torch.empty(S + 1, dtype=torch.int32, device=dev)
    benchsupport.synth_uniform(ctx, 0x5EED, F, P, F // S, 1, True, 1, wire, off, sf)
    payload = torch.empty(F * flen + 16 * F + 16, dtype=torch.uint8, device=dev)
    desc = torch.empty(F * 16, dtype=torch.uint8, device=dev)
    res = torch.empty(S * 16, dtype=torch.uint8, device=dev)
    state = torch.zeros(S * 8, dtype=torch.uint8, device=dev)
    ctx.reserve(F, S, F * flen)
    ctx.decode_device(snf4j_amd.decoder_cfg(False, False, 65536, True), wire, off, sf, state, payload, desc, res,
                      wire_len=F * flen)
    torch.cuda.synchronize(dev)
    del wire
    return validator_line(ctx, dev, desc, sf, payload, S, F, P, K)


def handshake_client_line(ctx, dev, steps, warmup, n=1 << 20, cpu_seconds=2.0):
    """Client opening handshakes (wsg_handshake_validate_batch_device): n servers'
    101 responses, each validated against the key its session sent (HandshakeDecoder
    in client mode + Handshaker.validate).  One lane per response.  cpu_baseline: the
    compiled C port on one host core, beside it on the job's cores and the Python
    restatement on one core (no JDK on the box)."""
    import base64
    import numpy as np
    import torch
    from oracle import handshake_oracle as H
    from snf4j_amd._lib import HS_EXPECTED_STRIDE, HS_RESULT_DTYPE, HsConfig
    tmpl = H.response(101, "Switching Protocols", [
        ("Server", "nginx/1.25.3"), ("Date", "Sat, 17 Oct 2026 00:00:00 GMT"), ("Connection", "upgrade"),
        ("Upgrade", "websocket"), ("Sec-WebSocket-Accept", "A" * 28)])
    L = len(tmpl)
    apos = tmpl.index(b"A" * 28)
    rng = np.random.default_rng(0xC11E)
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    keys = [base64.b64encode(r.tobytes()) for r in raw]
    k24 = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(n, 24)
    acc = np.frombuffer(b"".join(H.answer_key(k.decode()).encode() for k in keys), dtype=np.uint8).reshape(n, 28)
    buf = np.tile(np.frombuffer(tmpl, dtype=np.uint8), (n, 1))
    buf[:, apos:apos + 28] = acc
    resp = torch.from_numpy(buf.reshape(-1)).to(dev)
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    kd = torch.from_numpy(k24.reshape(-1).copy()).to(dev)
    exp = torch.empty(n * HS_EXPECTED_STRIDE, dtype=torch.uint8, device=dev)
    res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    cfg = HsConfig(65536, 0, 0, 0, 0)

    def step():
        ctx.handshake_validate_device(cfg, resp, off, kd, exp, res, n=n)

    step()
    torch.cuda.synchronize(dev)
    r = res.cpu().numpy().view(HS_RESULT_DTYPE)
    assert (r["kind"] == H.FINISHED).all(), "client handshake of the synthetic batch failed"
    for i in (0, 1, n // 2, n - 1):  # spot check against the restatement
        assert H.validate(buf[i].tobytes(), keys[i].decode())["kind"] == H.FINISHED, i
    el, kms, pipe = _timed(ctx, step, steps, warmup, dev, "k_hs_validate")
    alg = n * (L + 8 + 24 + 28 + 16)
    ach = alg / (kms / 1e3) / 1e9
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < cpu_seconds:
        H.validate(buf[done % n].tobytes(), keys[done % n].decode())
        done += 1
    t = time.perf_counter() - t0
    port1, portn = _hs_port_baselines(buf, n, L, keys=k24)
    return {"config": f"client handshake: {n} server responses of {L} B (101, random keys), "
                      "HandshakeDecoder(clientMode) + Handshaker.validate (key challenge, basic fields)",
            "value": round(n * steps / el / 1e6, 3), "unit": "M handshakes/s",
            "ms_per_step": round(el / steps * 1e3, 4),
            "roofline": {"kernel": "k_hs_validate", "bound": "per-lane serial parse + SHA-1 (not hbm)",
                         "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(ach / HBM_PEAK_GBS, 4), "alg_bytes_per_launch": alg,
                         "avg_launch_ms": round(kms, 4)},
            "cpu_baseline": port1, "cpu_baseline_threads": portn,
            "cpu_baseline_python": {"value": round(done / t / 1e6, 5), "unit": "M handshakes/s", "cores": 1,
                                    "kind": "port",
                                    "sample": f"{done} responses through the Python restatement "
                                              f"(oracle/handshake_oracle.py) in {t:.1f} s, 1 thread"},
            "pipeline_ms": pipe}


def e2e_stages_line(ctx, dev, K, W, n_s=4096, msgs=16, msg_bytes=4096, chunk=8192):
    """The native batcher with the decoders snf4j puts after "ws-decoder" when
    permessage-deflate is negotiated (FrameDecoder -> PerMessageDeflateDecoder ->
    FrameUtf8Validator, PerMessageDeflateExtension.java:316-326), end to end from host
    socket reads to host frames: per round one `chunk`-byte read of every session
    (wsg_batcher_feed_many), then wsg_batcher_flush_async (H2D, decode, inflate,
    validate, D2H), four flushes in flight.  Value: inflated bytes delivered per second."""
    import numpy as np
    import torch
    import snf4j_amd
    from benchsupport.synth import deflate_wire
    wire_np, starts, plain = deflate_wire(0x1F1A, n_s, msgs, msg_bytes)
    h_wire = torch.from_numpy(wire_np).pin_memory()
    hw = h_wire.numpy()
    base = hw.ctypes.data
    rounds = []
    pos, endv = starts[:-1].copy(), starts[1:].copy()
    while (pos < endv).any():
        live = np.nonzero(pos < endv)[0]
        ln = np.minimum(endv[live] - pos[live], chunk)
        rounds.append((live.astype(np.uint32), (base + pos[live]).astype(np.uint64), ln.astype(np.uint64)))
        pos[live] += chunk
    pctx = snf4j_amd.Context(dev.index, stream=torch.cuda.Stream(dev))
    apply_tuning(pctx)
    nb = snf4j_amd.NativeBatcher(n_s, clientMode=False, allowExtensions=True, maxPayloadLen=1 << 20, ctx=pctx)
    nb.set_stages(inflate=True, noContext=False, validate=True)
    # sized once, as WsgBatcher does (wsg_batcher_reserve, then _reserve_stages with its
    # STAGE_RATIO of 4 inflated bytes a wire byte): a round's reads plus carried partial
    # frames (messages are <= 4 KiB + header compressed); frames: a generous bound of one
    # a 64 B of a read (a flush beyond it would grow its buffers, as WsgBatcher's would)
    max_wire = max(int(lens.sum()) for _, _, lens in rounds) + n_s * (msg_bytes + 64)
    max_frames = n_s * (chunk // 64 + 2)
    nb.reserve(max_wire, max_frames)
    nb.reserve_stages(4 * max_wire, max_frames)
    times = []
    for rep in range(W + K):
        for s in range(n_s):
            nb.reset_session(s)  # the same streams again, from fresh sessions
        t0 = time.perf_counter()
        pending, out_bytes, n_fr = 0, 0, 0
        tw = tf = 0.0
        for sids, ptrs, lens in rounds:
            ta = time.perf_counter()
            nb.feed_many_ptrs(sids, ptrs, lens)
            tf += time.perf_counter() - ta
            if pending == BATCHER_MAX_INFLIGHT:
                ta = time.perf_counter()
                sfb, descb, _, resb, _ = nb.wait_raw()
                tw += time.perf_counter() - ta
                assert int(resb["error"].max()) == 0
                out_bytes += int(descb["payload_len"].astype(np.int64).sum())
                n_fr += len(descb)
                pending -= 1
            nb.flush_async()
            pending += 1
        while pending:
            ta = time.perf_counter()
            sfb, descb, _, resb, _ = nb.wait_raw()
            tw += time.perf_counter() - ta
            assert int(resb["error"].max()) == 0
            out_bytes += int(descb["payload_len"].astype(np.int64).sum())
            n_fr += len(descb)
            pending -= 1
        t = time.perf_counter() - t0
        assert out_bytes == plain and n_fr == n_s * msgs, (out_bytes, plain, n_fr)
        if rep >= W:
            times.append((t, tf, tw))
    nb.close()
    pctx.close()
    t, tf, tw = sorted(times)[len(times) // 2]
    return {"config": f"native batcher + stages (inflate -> validator), {n_s} sessions x {msgs} compressed TEXT "
                      f"messages x {msg_bytes} B, context takeover, {chunk} B reads ({wire_np.size / 1e6:.0f} MB wire "
                      f"-> {plain / 1e6:.0f} MB)",
            "value": round(plain / t / 2**30, 3), "unit": "GiB/s (inflated bytes, host to host)",
            "wire_GiB_per_s": round(wire_np.size / t / 2**30, 3), "ms_per_batch": round(t * 1e3, 3),
            "reps": K, "rounds": len(rounds), "feed_ms": round(tf * 1e3, 3), "wait_ms": round(tw * 1e3, 3),
            "api": "wsg_batcher_feed_many + wsg_batcher_flush_async/wait with wsg_batcher_set_stages"}


def e2e_stages_multi_line(ctx, dev, K, W, loops=(1, 2, 4), n_s=4096, msgs=16, msg_bytes=4096, chunk=8192):
    """The deployment shape the single-batcher lines avoid: L selector loops of one process on
    one device (WsgDevices puts them there when the node has fewer GPUs than loops), each with
    its own batcher, stage chain and context streams, driven from its own thread, the sessions
    split over the loops.  Each loop runs e2e_stages' round pattern over its sessions; value:
    inflated bytes of all loops / the wall time from the common start to the last loop's end,
    at the default GPU_MAX_HW_QUEUES."""
    import threading
    import numpy as np
    import torch
    import snf4j_amd
    from benchsupport.synth import deflate_wire
    wire_np, starts, plain = deflate_wire(0x1F1A, n_s, msgs, msg_bytes)
    h_wire = torch.from_numpy(wire_np).pin_memory()
    base = h_wire.numpy().ctypes.data
    out = {}
    for L in loops:
        per = n_s // L
        loops_state = []
        for li in range(L):
            s0, s1 = li * per, (li + 1) * per
            pos, endv = starts[s0:s1].copy(), starts[s0 + 1:s1 + 1].copy()
            rounds = []
            while (pos < endv).any():
                live = np.nonzero(pos < endv)[0]
                ln = np.minimum(endv[live] - pos[live], chunk)
                rounds.append((live.astype(np.uint32), (base + pos[live]).astype(np.uint64), ln.astype(np.uint64)))
                pos[live] += chunk
            pctx = snf4j_amd.Context(dev.index, stream=torch.cuda.Stream(dev))
            apply_tuning(pctx)
            nb = snf4j_amd.NativeBatcher(per, clientMode=False, allowExtensions=True, maxPayloadLen=1 << 20, ctx=pctx)
            nb.set_stages(inflate=True, noContext=False, validate=True)
            max_wire = max(int(lens.sum()) for _, _, lens in rounds) + per * (msg_bytes + 64)
            max_frames = per * (chunk // 64 + 2)
            nb.reserve(max_wire, max_frames)
            nb.reserve_stages(4 * max_wire, max_frames)
            loops_state.append((pctx, nb, rounds))

        def run(li, res):
            _, nb, rounds = loops_state[li]
            pending, ob = 0, 0
            for sids, ptrs, lens in rounds:
                nb.feed_many_ptrs(sids, ptrs, lens)
                if pending == BATCHER_MAX_INFLIGHT:
                    _, descb, _, resb, _ = nb.wait_raw()
                    assert int(resb["error"].max()) == 0
                    ob += int(descb["payload_len"].astype(np.int64).sum())
                    pending -= 1
                nb.flush_async()
                pending += 1
            while pending:
                _, descb, _, resb, _ = nb.wait_raw()
                assert int(resb["error"].max()) == 0
                ob += int(descb["payload_len"].astype(np.int64).sum())
                pending -= 1
            res[li] = ob

        times = []
        for rep in range(W + K):
            for _, nb, _ in loops_state:
                for s in range(per):
                    nb.reset_session(s)
            res = [0] * L
            ts = [threading.Thread(target=run, args=(li, res)) for li in range(L)]
            t0 = time.perf_counter()
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            t = time.perf_counter() - t0
            assert sum(res) == plain, (sum(res), plain)
            if rep >= W:
                times.append(t)
        for pctx, nb, _ in loops_state:
            nb.close()
            pctx.close()
        t = sorted(times)[len(times) // 2]
        out[str(L)] = {"GiB_per_s": round(plain / t / 2**30, 3), "ms_per_batch": round(t * 1e3, 3),
                       "sessions_per_loop": per}
    return {"config": f"native batcher + stages (inflate -> validator) on L loops of one process on one device, "
                      f"{n_s} sessions split over the loops, {msgs} compressed TEXT messages x {msg_bytes} B each, "
                      f"{chunk} B reads, each loop its own thread / batcher / stage chain / streams",
            "unit": "GiB/s (inflated bytes, host to host)", "loops": out,
            "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default")}


def e2e_encode_line(ctx, dev, K, W, n_s=64, msg_bytes=16 << 20, frame=65536, per_round=16):
    """The native encode batcher host to host on configs[4]'s shape (64 client sessions,
    a 16 MiB message each in 64 KiB fragments, FrameEncoder.java:69-120): per round
    (a loop iteration) every session queues `per_round` fragments
    (wsg_enc_batcher_add_many copies them into the pinned arena), then
    wsg_enc_batcher_flush_async; two flushes in flight, each waited view's wire bytes
    counted.  Value: wire bytes out per second."""
    import numpy as np
    import torch
    import snf4j_amd
    rng = np.random.default_rng(0xE4C)
    src = rng.integers(0, 256, msg_bytes, dtype=np.uint8)  # the same message bytes for every session
    nf = msg_bytes // frame
    # the batcher on a context of its own, as a selector loop's is (WsgBatcher), not on
    # the one the device-resident lines used
    pctx = snf4j_amd.Context(dev.index, stream=torch.cuda.Stream(dev))
    apply_tuning(pctx)
    eb = snf4j_amd.EncodeBatcher(n_s, True, ctx=pctx)
    masks = rng.integers(0, 256, (n_s, nf, 4), dtype=np.uint8)
    base = src.ctypes.data
    # a round's writes, session by session: fragments [r, r + per_round) of every session
    rounds = []
    for r in range(0, nf, per_round):
        idx = np.arange(r, min(nf, r + per_round))
        sids = np.repeat(np.arange(n_s, dtype=np.uint32), len(idx))
        fi = np.tile(idx, n_s)
        rounds.append((sids, np.where(fi == 0, 2, 0).astype(np.uint8),
                       np.where(fi == nf - 1, 0x80, 0).astype(np.uint8), masks[sids, fi],
                       (base + fi.astype(np.uint64) * frame).astype(np.uint64),
                       np.full(len(fi), frame, dtype=np.uint32)))
    times = []
    wire_total = 0
    for rep in range(W + K):
        t0 = time.perf_counter()
        pending, wb = 0, 0
        for sids, ops, fl, mk, ptrs, lens in rounds:
            eb.add_many_ptrs(sids, ops, fl, mk, ptrs, lens)
            if pending == 2:
                sf, off, wire = eb.wait_raw()
                wb += int(off[-1])
                pending -= 1
            eb.flush_async()
            pending += 1
        while pending:
            sf, off, wire = eb.wait_raw()
            wb += int(off[-1])
            pending -= 1
        t = time.perf_counter() - t0
        if rep >= W:
            times.append(t)
        wire_total = wb
    eb.close()
    pctx.close()
    exp = n_s * nf * (frame + 14)
    assert wire_total == exp, (wire_total, exp)
    t = float(np.median(times))
    return {"config": f"native encode batcher, configs[4] shape: {n_s} client sessions x {msg_bytes >> 20} MiB in "
                      f"{frame >> 10} KiB fragments, {per_round} fragments a session per flush, host to host",
            "value": round(wire_total / t / 2**30, 3), "unit": "GiB/s (wire out, host to host)",
            "ms_per_batch": round(t * 1e3, 3), "reps": K,
            "api": "per round wsg_enc_batcher_add_many + wsg_enc_batcher_flush_async/wait, two flushes in flight"}


def e2e_aggregate_line(ctx, dev, K, W, chunk=65536):
    """The native batcher with FrameAggregator after the decoder (wsg_batcher_set_stages
    aggregate; FrameAggregator.java:72-104) on configs[2]'s 4 GiB mixed batch, host to
    host: per round one `chunk`-byte read of every session, four flushes in flight;
    the decode's UTF-8 check stays fused.  Value: wire bytes fed per second."""
    import numpy as np
    import torch
    import snf4j_amd
    from benchsupport.synth import mixed_plan
    # configs[2]'s mix without the invalid UTF-8 (a failed session swallows the rest of its
    # input: with 1% bad messages most of the 4 GiB would never reach the aggregator)
    t, offh, sfh, wl, info = mixed_plan(0xC0F3, 1024, 4 << 30, bad_frac=0.0)
    n_s = 1024
    tab = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    wire = torch.zeros(wl + 64, dtype=torch.uint8, device=dev)
    benchsupport.synth_frames(ctx, tab, wire)
    del tab
    h_wire = torch.empty(wl, dtype=torch.uint8).pin_memory()
    h_wire.copy_(wire[:wl])
    del wire
    torch.cuda.empty_cache()
    hw = h_wire.numpy()
    base = hw.ctypes.data
    starts = offh[sfh[:-1].astype(np.int64)].astype(np.int64)
    ends = offh[sfh[1:].astype(np.int64)].astype(np.int64)
    rounds = []
    pos = starts.copy()
    while (pos < ends).any():
        live = np.nonzero(pos < ends)[0]
        ln = np.minimum(ends[live] - pos[live], chunk)
        rounds.append((live.astype(np.uint32), (base + pos[live]).astype(np.uint64), ln.astype(np.uint64)))
        pos[live] += chunk
    pctx = snf4j_amd.Context(dev.index, stream=torch.cuda.Stream(dev))
    apply_tuning(pctx)
    nb = snf4j_amd.NativeBatcher(n_s, clientMode=False, allowExtensions=False, maxPayloadLen=65536, ctx=pctx)
    nb.set_stages(inflate=False, validate=True, aggregate=True, maxAggregatedLength=16 << 20)
    times = []
    n_out = n_err = 0
    for rep in range(W + K):
        for s in range(n_s):
            nb.reset_session(s)
        t0 = time.perf_counter()
        pending, n_out, n_err = 0, 0, 0
        for sids, ptrs, lens in rounds:
            nb.feed_many_ptrs(sids, ptrs, lens)
            if pending == BATCHER_MAX_INFLIGHT:
                sfb, descb, _, resb, _ = nb.wait_raw()
                n_out += int(resb["n_delivered"].astype(np.int64).sum())
                n_err += int((resb["error"] != 0).sum())
                pending -= 1
            nb.flush_async()
            pending += 1
        while pending:
            sfb, descb, _, resb, _ = nb.wait_raw()
            n_out += int(resb["n_delivered"].astype(np.int64).sum())
            n_err += int((resb["error"] != 0).sum())
            pending -= 1
        tt = time.perf_counter() - t0
        if rep >= W:
            times.append(tt)
    nb.close()
    pctx.close()
    assert n_err == len(info["bad_sessions"]), (n_err, len(info["bad_sessions"]))
    tm = float(np.median(times))
    return {"config": f"native batcher + FrameAggregator stage, configs[2]'s mix ({wl / 2**30:.2f} GiB wire, 1024 sessions, "
                      f"10% of messages fragmented, no invalid UTF-8), {chunk} B reads, host to host",
            "value": round(wl / tm / 2**30, 3), "unit": "GiB/s (wire, host to host)", "ms_per_batch": round(tm * 1e3, 2),
            "frames_out": n_out, "sessions_failed": n_err, "reps": K, "rounds": len(rounds),
            "api": "wsg_batcher_feed_many + wsg_batcher_flush_async/wait with wsg_batcher_set_stages(aggregate)"}


EXTRA_LINES = {"configs1": line_configs1, "configs3": line_configs3, "configs2": line_configs2,
               "encode": line_encode, "validator": line_validator, "e2e_stages": e2e_stages_line,
               "e2e_stages_steady": lambda ctx, dev, K, W: e2e_stages_line(ctx, dev, K, W, msgs=64),
               "e2e_encode": e2e_encode_line, "e2e_aggregate": e2e_aggregate_line,
               "e2e_stages_multi": e2e_stages_multi_line,
               "inflate": lambda ctx, dev, K, W: inflate_line(ctx, dev, K, W),
               "deflate": lambda ctx, dev, K, W: deflate_line(ctx, dev, K, W),
               "handshake": lambda ctx, dev, K, W: handshake_line(ctx, dev, K, W),
               "hs_client": lambda ctx, dev, K, W: handshake_client_line(ctx, dev, K, W)}


def measure_extras(ctx, dev, args):
    """The other 1-GPU configurations of BASELINE.json, each a device-resident batch."""
    import torch
    out = []
    for name in ("configs1", "configs3", "configs2", "encode", "inflate", "deflate", "handshake", "hs_client"):
        out.append(EXTRA_LINES[name](ctx, dev, args.extra_steps, 2))
        torch.cuda.empty_cache()
    return out


def e2e_rate(ctx, cfg, wire, off, sf, n_s, wire_bytes, F, dev, reps=6):
    """Host-resident batches through the PCIe-inclusive path: GiB/s of wire.
    serial: pinned host -> H2D -> decode -> D2H, one batch at a time.
    pipelined: wsg_decode_batch_host_async, uploads / kernels / downloads on three
    streams, so batch i's D2H overlaps batch i+1's H2D and kernels (the JNI batcher's shape)."""
    import numpy as np
    import torch
    import snf4j_amd
    h_wire = torch.empty(wire_bytes, dtype=torch.uint8).pin_memory()
    h_wire.copy_(wire[:wire_bytes])
    h_off = off.cpu().pin_memory()
    h_sf = sf.cpu().pin_memory()
    pay_n = wire_bytes + 16 * F + 16
    out = {}
    # serial
    d_pay = torch.empty(pay_n, dtype=torch.uint8, device=dev)
    d_desc = torch.empty(F * 16, dtype=torch.uint8, device=dev)
    d_res = torch.empty(n_s * 16, dtype=torch.uint8, device=dev)
    d_state = torch.zeros(n_s * 8, dtype=torch.uint8, device=dev)
    h_pay = torch.empty(wire_bytes + 16 * F, dtype=torch.uint8).pin_memory()
    h_desc = torch.empty(F * 16, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        wire[:wire_bytes].copy_(h_wire, non_blocking=True)
        ctx.decode_device(cfg, wire, off, sf, d_state, d_pay, d_desc, d_res, wire_len=wire_bytes)
        h_pay.copy_(d_pay[:h_pay.numel()], non_blocking=True)
        h_desc.copy_(d_desc, non_blocking=True)
    torch.cuda.synchronize(dev)
    t = (time.perf_counter() - t0) / reps
    out["serial"] = {"GiB_per_s": round(wire_bytes / t / 2**30, 3), "ms_per_batch": round(t * 1e3, 3)}
    del d_pay, d_desc, d_res, d_state
    torch.cuda.empty_cache()
    # pipelined library host path (copy-in / kernel / copy-out streams, two staging slots)
    pctx = snf4j_amd.Context(dev.index, stream=torch.cuda.Stream(dev))
    apply_tuning(pctx)
    bufs = []
    for _ in range(2):
        bufs.append({"pay": torch.empty(wire_bytes + 16 * F, dtype=torch.uint8).pin_memory() if not bufs else None,
                     "desc": torch.empty(F * 16, dtype=torch.uint8).pin_memory(),
                     "res": torch.empty(n_s * 16, dtype=torch.uint8).pin_memory(),
                     "state": torch.zeros(n_s * 8, dtype=torch.uint8).pin_memory()})
    bufs[1]["pay"] = h_pay
    pctx.reserve(F, n_s, wire_bytes)
    for i in range(2):  # warm both staging slots
        b = bufs[i]
        pctx.decode_host_async(cfg, h_wire, h_off, h_sf, b["state"], b["pay"], b["desc"], b["res"])
    pctx.sync()
    t0 = time.perf_counter()
    for i in range(reps):
        b = bufs[i % 2]
        pctx.decode_host_async(cfg, h_wire, h_off, h_sf, b["state"], b["pay"], b["desc"], b["res"])
    pctx.sync()
    t = (time.perf_counter() - t0) / reps
    out["pipelined"] = {"GiB_per_s": round(wire_bytes / t / 2**30, 3), "ms_per_batch": round(t * 1e3, 3),
                        "api": "wsg_decode_batch_host_async"}
    # the native batcher (wsg_batcher_*): socket-read chunks of every session fed in,
    # frames delimited on the host, gathered to pinned staging, one device batch.
    # Loop-shaped: a round is one 64 KiB read of every session (wsg_batcher_feed_many,
    # sessions fed by several threads), then wsg_batcher_flush_async; two flushes in
    # flight, so a round's feeds and gather overlap the previous round's H2D, decode and
    # D2H.  Wire bytes of every round / the time from the first feed to the last wait.
    nb = snf4j_amd.NativeBatcher(n_s, ctx=pctx)
    hw = h_wire.numpy()
    offh, sfh = h_off.numpy(), h_sf.numpy()
    chunk = 65536
    starts = [int(offh[int(sfh[s])]) for s in range(n_s)]
    ends = [int(offh[int(sfh[s + 1])]) for s in range(n_s)]
    rounds = []  # (session ids, host addresses, lengths) of a round's reads, as a loop hands them over
    base = hw.ctypes.data
    pos = np.array(starts, dtype=np.int64)
    endv = np.array(ends, dtype=np.int64)
    while (pos < endv).any():
        live = np.nonzero(pos < endv)[0]
        ln = np.minimum(endv[live] - pos[live], chunk)
        rounds.append((live.astype(np.uint32), (base + pos[live]).astype(np.uint64), ln.astype(np.uint64)))
        pos[live] += chunk
    timing = None
    for rnd in range(2):  # round 0 sizes the batcher's buffers (pinned allocation); round 1 is timed
        if rnd == 1:
            for s in range(n_s):
                nb.reset_session(s)  # the same streams again, from fresh sessions
        t0 = time.perf_counter()
        pending, wb, n_fr, feed_t = 0, 0, 0, 0.0
        for sids, ptrs, lens in rounds:
            tf = time.perf_counter()
            nb.feed_many_ptrs(sids, ptrs, lens)
            feed_t += time.perf_counter() - tf
            if pending == BATCHER_MAX_INFLIGHT:
                sfb, descb, _, resb, w = nb.wait_raw()
                assert int(resb["error"].max()) == 0
                wb, n_fr, pending = wb + w, n_fr + len(descb), pending - 1
            nb.flush_async()
            pending += 1
        while pending:
            sfb, descb, _, resb, w = nb.wait_raw()
            assert int(resb["error"].max()) == 0
            wb, n_fr, pending = wb + w, n_fr + len(descb), pending - 1
        t2 = time.perf_counter()
        timing = (t0, t2, feed_t, wb, n_fr)
    t0, t2, feed_t, wb, n_fr = timing
    assert wb == wire_bytes and n_fr == F, (wb, wire_bytes, n_fr, F)
    out["native_batcher"] = {"GiB_per_s": round(wb / (t2 - t0) / 2**30, 3), "wire_bytes": wb,
                             "rounds": len(rounds), "total_s": round(t2 - t0, 4), "feed_s": round(feed_t, 4),
                             "feed_GiB_per_s": round(wb / feed_t / 2**30, 3),
                             "api": "per round: wsg_batcher_feed_many (one 64 KiB socket read per session, "
                                    "copied once into the open batch's pinned arena and framed in place, "
                                    "threaded by session) + wsg_batcher_flush_async (H2D, decode, D2H of the "
                                    "arena, no gather), four flushes in flight"}
    nb.close()
    out["drop_in_loop"] = e2e_loop_line(pctx, rounds, wire_bytes, F, n_s)
    pctx.close()
    out["path"] = "pinned host wire -> H2D -> decode -> D2H payload region + descriptors + results + state"
    return out


def e2e_loop_line(pctx, rounds, wire_bytes, F, n_s):
    """The drop-in's own call pattern (WsgBatcher.java, restated in snf4j_amd/loop.py):
    per loop iteration the reads are recorded, the flush task feeds them in one
    wsg_batcher_feed_many, delivers every earlier flush whose device work finished
    (waiting only when two are in flight), queues this one and hands its ticket to the
    completion thread, which re-enters the loop (executenf) when it is done.  The same
    socket reads as native_batcher (one 64 KiB read per session an iteration), wire
    bytes of all iterations / the time from the first read to the last delivery."""
    import numpy as np
    from benchsupport.selector import SelectorLoop, run_until_idle
    from snf4j_amd.loop import LoopBatcher
    got = {"wire": 0, "frames": 0}

    def deliver(_sid, views, _exc):
        _, desc, _, res, w = views
        assert int(res["error"].max()) == 0
        got["wire"] += w
        got["frames"] += len(desc)

    # WsgBatcher reserves its buffers at construction (wsg_batcher_reserve with its
    # maxWireLen / maxFrames): a flush's wire is an iteration's reads plus the partial
    # frames carried into it, its frames at most one a FLEN of that
    flen = wire_bytes // F
    max_wire = max(int(lens.sum()) for _, _, lens in rounds) + n_s * flen
    max_frames = max_wire // flen + n_s
    best = None
    for rnd in range(3):  # round 0 warms up; the best of two timed rounds
        loop = SelectorLoop()
        lb = LoopBatcher(loop, n_s, deliver, ctx=pctx, raw=True, max_wire=max_wire, max_frames=max_frames,
                         max_inflight=BATCHER_MAX_INFLIGHT)
        got["wire"] = got["frames"] = 0
        t0 = time.perf_counter()
        for sids, ptrs, lens in rounds:
            loop.run_iteration([lambda s=sids, p=ptrs, ln=lens: lb.enqueue_many_ptr(s, p, ln)])
        run_until_idle(loop, lb, timeout=120)
        t = time.perf_counter() - t0
        st = dict(lb.stats)
        lb.close()
        assert got["wire"] == wire_bytes and got["frames"] == F, (got, wire_bytes, F)
        if rnd and (best is None or t < best[0]):
            best = (t, st)
    t, st = best
    return {"GiB_per_s": round(wire_bytes / t / 2**30, 3), "total_s": round(t, 4), "iterations": len(rounds),
            "flushes": st["flushes"], "collected_in_a_later_iteration": st["collected_later"],
            "collected_blocking": st["collected_blocking"],
            "api": "WsgBatcher's scheduling (snf4j_amd/loop.py): per iteration one wsg_batcher_feed_many of the "
                   "recorded reads, finished flushes collected via wsg_batcher_await(0), flush_async + a "
                   "completion thread re-entering the loop; the rate a Java selector loop gets"}


if __name__ == "__main__":
    main()
