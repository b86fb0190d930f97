"""bench.py's launcher contract (CPU only, nothing touches a GPU): under a launcher,
--gpus must equal WORLD_SIZE, so a line can never report fewer GPUs than asked for."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True,
                          text=True, timeout=120)


def test_gpus_must_match_world_size():
    r = _run(["--gpus", "8"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 8 but WORLD_SIZE=1" in r.stderr


def test_config_choices_and_overrides():
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--config", "3"]
        a = bench.parse()
        assert (a.frames, a.payload, a.sessions, a.binary) == (8 << 20, 4096, 1024, False)
        sys.argv = ["bench.py", "--config", "1", "--frames", "4096"]
        a = bench.parse()
        assert (a.frames, a.payload, a.sessions, a.binary) == (4096, 1024, 256, True)
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert (a.frames, a.payload, a.sessions, a.binary, a.gpus) == (1 << 20, 4096, 1024, False, None)
    finally:
        sys.argv = argv


def test_full_and_dump_outputs_options():
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
        sys.argv = ["bench.py", "--full", "--dump-outputs", "somewhere"]
        a = bench.parse()
        assert (a.full, a.dump_outputs) == (True, "somewhere")
    finally:
        sys.argv = argv


def test_dump_outputs_files(tmp_path):
    """dump_outputs on host tensors laid out as decode_device leaves them: float .npy files,
    the sampled payload bytes are the frames' own, and a second dump is identical."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from snf4j_amd._lib import DESC_DTYPE, RESULT_DTYPE
    F, S, P = 3000, 7, 37  # more frames than bench.DUMP_PAYLOAD_FRAMES, odd payload length
    rng = np.random.default_rng(1)
    d = np.zeros(F, dtype=DESC_DTYPE)
    d["payload_off"] = np.arange(F, dtype=np.uint64) * 48 + 5
    d["payload_len"], d["opcode"], d["flags"] = P, 1, 0x80
    r = np.zeros(S, dtype=RESULT_DTYPE)
    r["n_delivered"], r["detail"] = np.arange(S), -1
    pay = rng.integers(0, 256, F * 48 + 64, dtype=np.uint8)
    st = rng.integers(0, 256, S * 8, dtype=np.uint8)
    t = [torch.from_numpy(x.view(np.uint8).copy()) for x in (pay, d, r, st)]
    bench.dump_outputs(str(tmp_path / "a"), *t, F)
    bench.dump_outputs(str(tmp_path / "b"), *t, F)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "payload_bytes.npy" in names
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, np.load(tmp_path / "b" / (n + ".npy"))), n
    assert np.array_equal(got["frames"], np.arange(F)) and np.array_equal(got["desc_payload_off"], d["payload_off"])
    assert np.array_equal(got["result_detail"], r["detail"]) and np.array_equal(got["state"], st.reshape(S, 8))
    pf = got["payload_frames"].astype(np.int64)
    assert len(pf) == bench.DUMP_PAYLOAD_FRAMES and len(set(pf)) == len(pf)
    exp = np.concatenate([pay[int(d["payload_off"][k]):][:P] for k in pf])
    assert np.array_equal(got["payload_bytes"], exp)


def test_cpu_threads_from_affinity(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    aff = len(os.sched_getaffinity(0))
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert bench.cpu_threads()[0] == aff
    if aff > 1:
        monkeypatch.setenv("OMP_NUM_THREADS", "1")
        assert bench.cpu_threads()[0] == 1


def test_bench_inflight_limit_is_the_library_one():
    import bench
    from snf4j_amd import _lib
    assert bench.BATCHER_MAX_INFLIGHT == _lib.BATCHER_MAX_INFLIGHT
