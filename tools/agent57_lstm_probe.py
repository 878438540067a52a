"""Probe: Agent57's recurrent layer on libsrlx's LSTM kernels ("srlx") next to torch.nn.LSTM ("torch"), the measurement that decides QNetwork.lstm_backend's default.

    python tools/agent57_lstm_probe.py --out profiles/agent57_lstm_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/agent57_lstm_probe.py --trace-loop      # a run of its own, no counters

Three GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the
GPU).  Inside a step the two arms run in ONE process, interleaved three times (srlx, torch, srlx, torch, ...), after one untimed call of each arm (allocation,
MIOpen's solver search); every timing ends in a device synchronise:
  golden      one whole Trainer.train() at the shape of tests/golden/train_step_agent57.npz (B = 8, burn-in 2 + sequence 3 + 1, H = 16, TinyImg-sized frames)
  atari       one whole Trainer.train() at set_atari_config()'s shape (B = 64, 40 + 80 + 1 steps, H = 512, 84 x 84 frames: I = 7744 + 1 + 32)
  lstm_alone  the layer's forward + backward alone on synthetic tensors of the Atari shape
The default rule (README): "srlx" iff atari.srlx_ms_mean <= 1.10 * atari.torch_ms_mean of the same run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = dict(golden=300, atari=900, lstm_alone=420)  # seconds per child
ARMS = ("srlx", "torch")


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _interleaved(fns, rounds=3):
    """fns: {arm: callable}.  One untimed call each, then `rounds` interleaved timed calls."""
    for f in fns.values():
        f()
    runs = {a: [] for a in fns}
    for _ in range(rounds):
        for a, f in fns.items():
            runs[a].append(_timed(f))
    res = {a + "_ms": r for a, r in runs.items()}
    res.update({a + "_ms_mean": sum(r) / len(r) for a, r in runs.items()})
    res["srlx_over_torch"] = res["srlx_ms_mean"] / res["torch_ms_mean"]
    return res


def _trainer(kind, backend):
    """A set-up Agent57 trainer whose memory hands out one fixed synthetic batch; returns (trainer, shape description)."""
    import numpy as np
    import torch

    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import agent57
    from simple_distributed_rl_amd.base.context import RunContext

    if kind == "atari":
        rl = agent57.Config()
        rl.set_atari_config()
        rl.window_length = 1
        env = srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(episode_len=200))
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from simple_distributed_rl_amd.base.env import registration
        from test_plugin_surface import TinyImg  # noqa: F401

        registration.register("TinyImg", "test_plugin_surface:TinyImg", check_duplicate=False)
        rl = agent57.Config(batch_size=8, actor_num=4, target_model_update_interval=5, lr_ext=0.001, lr_int=0.002, lstm_units=16, burnin=2, sequence_length=3)
        rl.window_length = 1
        rl.hidden_block.set_dueling_network((16,))
        env = srl.EnvConfig("TinyImg")
    rl.memory.capacity, rl.memory.warmup_size, rl.memory.compress = 1000, rl.batch_size, False
    runner = srl.Runner(env, rl)
    runner.set_device("cuda:0")
    runner.set_seed(1)
    param, trainer = runner.parameter, runner.trainer
    ctx = RunContext(runner.env_config, rl)
    ctx.setup_device()
    trainer.setup(ctx)
    nets = (param.q_ext_online, param.q_ext_target, param.q_int_online, param.q_int_target)
    for net in nets:
        net.lstm_backend = backend
    rng = np.random.default_rng(0)
    B, L, S, A, H = rl.batch_size, rl.burnin + rl.sequence_length + 1, rl.sequence_length, rl.action_space.n, rl.lstm_units
    obs = tuple(rl.observation_space.shape)
    eye = np.identity(A, dtype=int)
    hid = lambda: [rng.standard_normal((1, H)).astype(np.float32) * 0.1, rng.standard_normal((1, H)).astype(np.float32) * 0.1]  # noqa: E731
    batches = [[list(rng.random((L,) + obs, dtype=np.float32)), [eye[a] for a in rng.integers(0, A, L)], list(rng.integers(-1, 2, L).astype(np.float64)),
                list(rng.random(L)), [1] * S, int(rng.integers(0, rl.actor_num)), [[] for _ in range(S)], hid(), hid()] for _ in range(B)]
    weights = np.ones(B, np.float32)
    trainer.memory.sample = lambda *a, **k: (batches, weights, list(range(B)))
    trainer.memory.update = lambda *a, **k: None
    trainer.train_count = 1
    torch.manual_seed(0)
    return trainer, nets, dict(batch=B, steps=L, burnin=rl.burnin, lstm_units=H, lstm_inputs=nets[0].lstm_layer.input_size, observation=list(obs), actions=A)


def _step_trainer(kind):
    arms = {}
    shape = None
    for backend in ARMS:
        trainer, nets, shape = _trainer(kind, backend)

        def run(trainer=trainer, nets=nets, backend=backend):
            trainer.train()
            assert all(n.lstm_path == backend for n in nets), [n.lstm_path for n in nets]
        arms[backend] = run
    return dict(what="one whole Trainer.train() (host batch assembly included), ms", shape=shape, **_interleaved(arms))


def _step_lstm_alone():
    import torch

    from simple_distributed_rl_amd.device.lstm import SrlxLstm

    B, T, I, H = 64, 121, 7744 + 1 + 32, 512
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    layer = torch.nn.LSTM(I, H, batch_first=True).to(dev)  # the layer alone, without the image block and the head
    x = torch.randn(B, T, I, device=dev).requires_grad_(True)
    hid = (torch.randn(1, B, H, device=dev) * 0.1, torch.randn(1, B, H, device=dev) * 0.1)
    dy = torch.randn(B, T, H, device=dev)
    srlx = SrlxLstm()
    assert srlx.serves(layer, x)
    arms = {}
    for backend in ARMS:
        def run(backend=backend):
            layer.zero_grad()
            x.grad = None
            y, _ = srlx(layer, x, hid) if backend == "srlx" else layer(x, hid)
            y.backward(dy)
        arms[backend] = run
    return dict(what="LSTM forward + backward alone (dx and the four parameter gradients), ms", shape=dict(batch=B, steps=T, lstm_inputs=I, lstm_units=H), **_interleaved(arms))


def _trace_loop(steps):
    import torch

    trainer, nets, _ = _trainer("atari", "srlx")
    for _ in range(steps):
        trainer.train()
    torch.cuda.synchronize()


def run_steps(script, limits, names, out, rule):
    """The parent's part of a probe (this one and tools/agent57_inblock_probe.py): every step of `names` as a child of `script` under its limit, results merged
    into the JSON file `out`, the default `rule` applied to the atari step; exits with status 1 when a step failed (nothing more was started on the GPU)."""
    res = json.load(open(out)) if out and os.path.exists(out) else {}  # steps measured by an earlier call stay
    for step in names.split(","):
        t0 = time.time()
        print("step %s (limit %d s)" % (step, limits[step]), flush=True)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(script), "--child", step], capture_output=True, text=True, timeout=limits[step], cwd=ROOT)
        except subprocess.TimeoutExpired:
            res[step] = dict(error="no result within %d s" % limits[step])
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE-JSON ")]
        if p.returncode != 0 or not line:
            res[step] = dict(error="exit status %d" % p.returncode, stderr=p.stderr[-2000:])
            break
        res[step] = dict(json.loads(line[-1][len("PROBE-JSON "):]), wall_s=time.time() - t0)
    if "atari" in res and "srlx_over_torch" in res["atari"]:
        res["default_rule"] = dict(rule=rule, srlx_over_torch=res["atari"]["srlx_over_torch"], default="srlx" if res["atari"]["srlx_over_torch"] <= 1.10 else "torch")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    if any("error" in v for v in res.values() if isinstance(v, dict)):
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="golden,atari,lstm_alone")
    ap.add_argument("--child", default=None, help="(internal) run one GPU step in this process and print its JSON")
    ap.add_argument("--trace-loop", action="store_true", help="three Atari-shape trainer steps on the srlx backend, for a profiler")
    a = ap.parse_args()
    if a.trace_loop:
        return _trace_loop(3)
    if a.child:
        res = _step_lstm_alone() if a.child == "lstm_alone" else _step_trainer(a.child)
        print("PROBE-JSON " + json.dumps(res))
        return
    run_steps(__file__, LIMITS, a.steps, a.out, "lstm_backend defaults to 'srlx' iff the Atari-shape trainer step with it is at most 1.10 x the nn.LSTM arm's in this run")


if __name__ == "__main__":
    main()
