"""Probe: the R2D2 plugin's trainer step with its recurrent layer on libsrlx ("srlx") next to torch.nn.LSTM ("torch") -- the measurement that decides
r2d2.QNetwork.lstm_backend's default -- and the new target kernel next to Agent57's at the same shape.

    python tools/r2d2_probe.py --out profiles/r2d2_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/r2d2_probe.py --trace-loop      # a run of its own, no counters

Three GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the
GPU; the parent's part is tools/agent57_lstm_probe.py:run_steps).  Inside a trainer step the two arms run in ONE process, interleaved three times, after one
untimed call of each arm; every timing ends in a device synchronise:
  atari    one whole Trainer.train() at set_atari_config()'s shape (B = 64, 40 + 80 + 1 steps, H = 512, 84 x 84 frames, 18 actions)
  default  one whole Trainer.train() at r2d2.Config()'s defaults on a flat observation (Grid: B = 32, 5 + 5 + 1 steps, H = 512, 4 actions)
  kernel   srlx_r2d2_seq_td at (B, S, A) = (64, 80, 18) and srlx_agent57_seq_td at the same shape as algorithms/agent57.py launches it: 200 back-to-back
           calls each between two events, after 20 untimed ones, three times interleaved
The default rule (README): "srlx" iff atari.srlx_ms_mean <= 1.10 * atari.torch_ms_mean of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from agent57_lstm_probe import ARMS, _interleaved, run_steps  # noqa: E402

LIMITS = dict(atari=600, default=240, kernel=120)  # seconds per child


def _trainer(kind, backend):
    """A set-up R2D2 trainer whose memory hands out one fixed synthetic batch; returns (trainer, nets, shape description)."""
    import numpy as np
    import torch

    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import r2d2
    from simple_distributed_rl_amd.base.context import RunContext

    rl = r2d2.Config()
    if kind == "atari":
        rl.set_atari_config()
        env = srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(episode_len=200, n_actions=18))
    else:
        env = srl.EnvConfig("Grid")
    rl.memory.capacity, rl.memory.warmup_size, rl.memory.compress = 1000, rl.batch_size, False
    rl.memory.set_replay_buffer()
    runner = srl.Runner(env, rl)
    runner.set_device("cuda:0")
    runner.set_seed(1)
    param, trainer = runner.parameter, runner.trainer
    ctx = RunContext(runner.env_config, rl)
    ctx.setup_device()
    trainer.setup(ctx)
    nets = (param.q_online, param.q_target)
    for net in nets:
        net.lstm_backend = backend
    rng = np.random.default_rng(0)
    B, L, S, A, H = rl.batch_size, rl.burnin + rl.sequence_length + 1, rl.sequence_length, rl.action_space.n, rl.lstm_units
    obs = tuple(rl.observation_space.shape)
    batches = [dict(states=list(rng.random((L,) + obs, dtype=np.float32)), actions=[int(a) for a in rng.integers(0, A, S)],
                    probs=[float(p) for p in rng.uniform(0.1, 1.0, S)], rewards=[float(r) for r in rng.integers(-1, 2, S)], dones=[False] * S,
                    invalid_actions=[[] for _ in range(S + 1)],
                    hidden_states=[rng.standard_normal(H).astype(np.float32) * 0.1, rng.standard_normal(H).astype(np.float32) * 0.1]) for _ in range(B)]
    weights = np.ones(B, np.float32)
    trainer.memory.sample = lambda *a, **k: (batches, weights, list(range(B)))
    trainer.memory.update = lambda *a, **k: None
    trainer.train_count = 1
    torch.manual_seed(0)
    return trainer, nets, dict(batch=B, steps=L, burnin=rl.burnin, lstm_units=H, lstm_inputs=nets[0].lstm_layer.input_size, observation=list(obs), actions=A)


def _step_trainer(kind):
    arms, shape = {}, None
    for backend in ARMS:
        trainer, nets, shape = _trainer(kind, backend)

        def run(trainer=trainer, nets=nets, backend=backend):
            trainer.train()
            assert nets[0].lstm_path == backend, nets[0].lstm_path
        arms[backend] = run
    return dict(what="one whole Trainer.train() (host batch assembly included), ms", shape=shape, **_interleaved(arms))


def _step_kernel():
    import torch

    from simple_distributed_rl_amd.algorithms._device_ops import TdOps

    B, S, A = 64, 80, 18
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    q, qt, rewards, weights = r(B, S + 1, A), r(B, S + 1, A), r(B, S), torch.ones(B, device=dev)
    actions = torch.randint(0, A, (B, S), generator=g).to(torch.int32).to(dev)
    mu = (torch.rand(B, S, generator=g) * 0.9 + 0.1).to(dev)
    dones_u8, undone_f32 = torch.zeros((B, S), dtype=torch.uint8, device=dev), torch.ones((B, S), device=dev)
    discounts = torch.full((B,), 0.997, device=dev)
    ops = TdOps(dev)
    calls = {  # R2D2 with retrace on (the costlier path: the policy row is scanned too); Agent57 as its trainer calls it (no invalid mask in the batch)
        "r2d2_seq_td": lambda: ops.r2d2_seq_td(q, qt, actions, mu, rewards, dones_u8, None, weights, 0.997, 0.95, True, True, True),
        "agent57_seq_td": lambda: ops.agent57_seq_td(q, qt, actions, rewards, undone_f32, None, discounts, weights, 0.95, True, True),
    }
    us = {k: [] for k in calls}
    for f in calls.values():
        for _ in range(20):
            f()
    for _ in range(3):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(200):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(1e3 * e0.elapsed_time(e1) / 200)
    return dict(what="microseconds per call, 200 back-to-back calls between two events (launch overhead and the wrapper's allocations included; r2d2_seq_td is "
                     "two launches, agent57_seq_td a memset and one launch)", shape=dict(batch=B, seq_len=S, actions=A),
                **{k + "_us": v for k, v in us.items()}, **{k + "_us_mean": sum(v) / len(v) for k, v in us.items()})


def _trace_loop(steps):
    import torch

    trainer, nets, _ = _trainer("atari", "srlx")
    for _ in range(steps):
        trainer.train()
    _step_kernel()  # Agent57's kernel at the same shape lands in the same trace
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="atari,default,kernel")
    ap.add_argument("--child", default=None, help="(internal) run one GPU step in this process and print its JSON")
    ap.add_argument("--trace-loop", action="store_true", help="three Atari-shape trainer steps on the srlx backend and the kernel step, for a profiler")
    a = ap.parse_args()
    if a.trace_loop:
        return _trace_loop(3)
    if a.child:
        res = _step_kernel() if a.child == "kernel" else _step_trainer(a.child)
        print("PROBE-JSON " + json.dumps(res))
        return
    run_steps(__file__, LIMITS, a.steps, a.out, "r2d2.QNetwork.lstm_backend defaults to 'srlx' iff the Atari-shape trainer step with it is at most 1.10 x the "
                                                "nn.LSTM arm's in this run")


if __name__ == "__main__":
    main()
