"""Probe: Agent57's replay with `agent57.Memory.sequence_store = "device"` (frame ring in HBM, one gather launch per batch) next to the "host" store
with and without item compression, the measurement that a later change decides the default from.

    python tools/agent57_seqstore_probe.py --out profiles/agent57_seqstore_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/agent57_seqstore_probe.py --trace-loop      # a run of its own, no counters

Two GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the GPU).
Inside a step the arms run in ONE process, interleaved three times after one untimed call of each arm; every timing is a host clock that ends in a device
synchronise:
  atari   set_atari_config()'s shape (B = 64, 40 + 80 + 1 steps, H = 512, 84 x 84 frames).  Three memories (device, host with compress=False, host with the default
          compress=True) are filled by the SAME stream of worker-shaped adds (consecutive windows share their frame objects; frames are random bytes / 255, the
          worst case for zlib).  Timed: one `memory.add`, and one whole `Trainer.train()` that samples from its memory.  The memories hold 512 sequences, so the
          device arm's ring (21 MB) is cache-resident here; `gather` below is the HBM-resident case.
  gather  srlx_seq_gather alone on a store of 20 000 sequences (a 571 MB ring, beyond the 256 MB Infinity Cache) whose frame tables point at random distinct rows,
          B = 64: device-event time, bytes read + written from the shapes, the share of the 8 TB/s line, and a plain `copy_` of the states tensor next to it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = dict(atari=900, gather=300)  # seconds per child
ARMS = ("device", "host", "host_compress")
HBM_LINE = 8.0e12  # bytes / s: the line the project quotes for its bandwidth kernels


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _interleaved(fns, rounds=3):
    for f in fns.values():
        f()
    runs = {a: [] for a in fns}
    for _ in range(rounds):
        for a, f in fns.items():
            runs[a].append(_timed(f))
    res = {a + "_ms": r for a, r in runs.items()}
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    return res


def _worker_stream(L, S, A, H, obs, actors, episode_len, seed=0):
    """Items shaped like `agent57.Worker._add_memory`'s, endlessly: windows shifted by one step, shared frame objects, dummy padding around episodes."""
    import numpy as np

    rng = np.random.default_rng(seed)
    dummy = np.zeros(obs, np.float32)
    eye = np.identity(A, dtype=int)
    fresh = lambda: rng.integers(0, 256, obs, dtype=np.uint8).astype(np.float32) / 255  # noqa: E731
    hid = lambda: [rng.standard_normal((1, H)).astype(np.float32) * 0.1, rng.standard_normal((1, H)).astype(np.float32) * 0.1]  # noqa: E731
    while True:
        actor = int(rng.integers(0, actors))
        cols = [[dummy] * (L - 1) + [fresh()], [eye[rng.integers(A)] for _ in range(L)], [0.0] * L, [0.0] * L, [1] * S, [[] for _ in range(S)]]
        h_ext, h_int = [hid() for _ in range(L)], [hid() for _ in range(L)]
        for t in range(episode_len + L - 1):
            step = t < episode_len
            vals = (fresh(), eye[rng.integers(A)], float(rng.integers(-1, 2)), float(rng.random()), 0 if t == episode_len - 1 else 1, []) if step else \
                (dummy, eye[rng.integers(A)], 0.0, 0.0, 0, [])
            cols = [c[1:] + [v] for c, v in zip(cols, vals)]
            h_ext, h_int = h_ext[1:] + ([hid()] if step else []), h_int[1:] + ([hid()] if step else [])
            yield [cols[0][:], cols[1][:], cols[2][:], cols[3][:], cols[4][:], actor, cols[5][:], h_ext[0], h_int[0]]


def _atari_trainer(arm, capacity):
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import agent57
    from simple_distributed_rl_amd.base.context import RunContext

    rl = agent57.Config()
    rl.set_atari_config()
    rl.window_length = 1
    rl.memory.capacity, rl.memory.warmup_size, rl.memory.compress = capacity, rl.batch_size, arm == "host_compress"
    agent57.Memory.sequence_store = "device" if arm == "device" else "host"
    runner = srl.Runner(srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(episode_len=200)), rl)
    runner.set_device("cuda:0")
    runner.set_seed(1)
    trainer = runner.trainer
    agent57.Memory.sequence_store = "host"
    ctx = RunContext(runner.env_config, rl)
    ctx.setup_device()
    trainer.setup(ctx)
    trainer.train_count = 1
    return trainer, rl


def _step_atari():
    import torch

    capacity, fill, timed_adds = 512, 320, 32
    trainers = {arm: _atari_trainer(arm, capacity) for arm in ARMS}
    rl = trainers["device"][1]
    B, L, S, A, H = rl.batch_size, rl.burnin + rl.sequence_length + 1, rl.sequence_length, rl.action_space.n, rl.lstm_units
    obs = tuple(rl.observation_space.shape)
    stream = _worker_stream(L, S, A, H, obs, rl.actor_num, episode_len=150)
    for _ in range(fill):  # the same items, the same objects, into all three memories
        item = next(stream)
        for arm in ARMS:
            trainers[arm][0].memory.add(item, None)
    torch.manual_seed(0)
    store = trainers["device"][0].memory._store

    def adds(arm):
        def run():
            for item in batch_of_items:
                trainers[arm][0].memory.add(item, None)
        return run

    add_runs = {arm: [] for arm in ARMS}
    h2d0, uploads0, serial0 = store.h2d_bytes, store.ledger.uploads, store.ledger.serial
    for rnd in range(4):  # round 0 untimed
        batch_of_items = [next(stream) for _ in range(timed_adds)]
        for arm in ARMS:
            ms = _timed(adds(arm)) / timed_adds
            if rnd:
                add_runs[arm].append(ms)
    n_adds = store.ledger.serial - serial0
    add = {arm + "_ms_per_add": r for arm, r in add_runs.items()}
    add.update({arm + "_ms_per_add_mean": sum(r) / len(r) for arm, r in add_runs.items()})
    frame_bytes = 4 * store.stride
    add.update(what="one memory.add of a worker-shaped window, host clock ending in a device synchronise, mean over %d consecutive adds, ms" % timed_adds,
               device_h2d_bytes_per_add=(store.h2d_bytes - h2d0) / n_adds, device_new_frames_per_add=(store.ledger.uploads - uploads0) / n_adds,
               host_h2d_bytes_per_add=0, host_h2d_bytes_per_update=B * L * frame_bytes, device_h2d_bytes_per_update=8 * B, item_frame_bytes=L * frame_bytes)
    step = _interleaved({arm: trainers[arm][0].train for arm in ARMS})
    step.update(what="one whole Trainer.train() sampling from its memory (batch assembly included), ms",
                shape=dict(batch=B, steps=L, burnin=rl.burnin, lstm_units=H, observation=list(obs), actions=A, memory_capacity=capacity, sequences_held=min(capacity, fill + 4 * timed_adds)))
    step["device_over_host"] = step["device_ms_mean"] / step["host_ms_mean"]
    step["device_over_host_compress"] = step["device_ms_mean"] / step["host_compress_ms_mean"]
    return dict(trainer_step=step, add=add)


def _big_store(capacity=20000):
    import torch

    from simple_distributed_rl_amd.device.sequence_store import DeviceSequenceStore

    L, S, A, H, obs = 121, 80, 18, 512, (84, 84, 1)
    store = DeviceSequenceStore("cuda:0", capacity, L, S, A, H, obs)
    store.ring.uniform_()
    F = store.ledger.frame_capacity
    g = torch.Generator(device="cpu").manual_seed(0)
    store.records[:, :L] = torch.randint(0, F, (capacity, L), generator=g, dtype=torch.int32).to(store.device)
    idx = torch.randint(0, capacity, (64,), generator=g, dtype=torch.int64).to(store.device)
    d = store.device
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=d)  # noqa: E731
    B = 64
    out = dict(states=f32(B, L, *obs), act_idx=torch.empty((B, L), dtype=torch.int64, device=d), r_ext=f32(B, L), r_int=f32(B, L), dones=f32(B, S),
               invalid=torch.empty((B, S, A), dtype=torch.uint8, device=d), actor=torch.empty(B, dtype=torch.int64, device=d), h_ext=f32(B, H), c_ext=f32(B, H),
               h_int=f32(B, H), c_int=f32(B, H))
    return store, idx, out


def _event_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def _step_gather():
    import torch

    store, idx, out = _big_store()
    lay = store.layout
    B = int(idx.shape[0])
    src = torch.rand_like(out["states"])
    dst = torch.empty_like(src)
    moved = 2 * out["states"].numel() * 4 + B * (4 * lay.dwords + sum(t.numel() * t.element_size() for k, t in out.items() if k != "states"))
    res = dict(what="srlx_seq_gather alone and a plain copy_ of the states tensor, device-event ms (each value one launch), interleaved three times",
               shape=dict(batch=B, steps=lay.L, frame_elems=store.frame_elems, ring_rows=store.ledger.frame_capacity, ring_bytes=store.ring.numel() * 4),
               bytes_read_plus_written=moved, copy_bytes_read_plus_written=2 * src.numel() * 4, gather_ms=[], copy_ms=[])
    for _ in range(3):
        res["gather_ms"] += _event_ms(lambda: store.gather_into(idx, out), 5)
        res["copy_ms"] += _event_ms(lambda: dst.copy_(src), 5)
    for k, nbytes in (("gather", moved), ("copy", res["copy_bytes_read_plus_written"])):
        ms = sorted(res[k + "_ms"])[len(res[k + "_ms"]) // 2]
        res[k + "_ms_median"] = ms
        res[k + "_tb_per_s"] = nbytes / (ms * 1e-3) / 1e12
        res[k + "_share_of_8tb_line"] = nbytes / (ms * 1e-3) / HBM_LINE
    return res


def _trace_loop(reps):
    import torch

    store, idx, out = _big_store()
    for _ in range(reps):
        store.gather_into(idx, out)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="atari,gather")
    ap.add_argument("--child", default=None, help="(internal) run one GPU step in this process and print its JSON")
    ap.add_argument("--trace-loop", action="store_true", help="ten Atari-shape gather launches on the HBM-resident store, for a profiler")
    a = ap.parse_args()
    if a.trace_loop:
        return _trace_loop(10)
    if a.child:
        print("PROBE-JSON " + json.dumps(_step_gather() if a.child == "gather" else _step_atari()))
        return
    res = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}  # steps measured by an earlier call stay
    for step in a.steps.split(","):
        t0 = time.time()
        print("step %s (limit %d s)" % (step, LIMITS[step]), flush=True)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=LIMITS[step], cwd=ROOT)
        except subprocess.TimeoutExpired:
            res[step] = dict(error="no result within %d s" % LIMITS[step])
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE-JSON ")]
        if p.returncode != 0 or not line:
            res[step] = dict(error="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            break
        res[step] = dict(json.loads(line[-1][len("PROBE-JSON "):]), wall_s=time.time() - t0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    if any("error" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


if __name__ == "__main__":
    main()
