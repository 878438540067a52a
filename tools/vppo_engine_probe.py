"""Probe: the V-PPO device engine (device/vppo_engine.py) next to `Runner.train()` on the plugin path, both on ppo_v.Config() and CartPole, past
the warm-up.

    python tools/vppo_engine_probe.py --out profiles/vppo_engine_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o act --output-format csv -- python tools/vppo_engine_probe.py --trace-loop      # a run of its own, no counters

All arms run in ONE process and are interleaved three times.  The plugin arm is ONE `Runner.train()` call: an `on_step_end` hook times three segments of SEGMENT
environment steps after step warmup_size + 200, and between them runs one round of every engine arm.  An engine arm is built beforehand and run, untimed, past
its warm-up and its first update; a round is ROUND whole `step(learner_updates=1)` calls ending in a device synchronise.  After the timed rounds every engine
runs PHASE_STEPS more lock-steps with `phase_times` on (the engine then synchronises around `actor_step` and `learner_step`): their host milliseconds per call.
The yardstick of the engine is the plugin arm of the same run.
--trace-loop runs, at 1024 rows of 4 floats through ppo_v.Config()'s network (trunk 64-64, value block 64, no policy block, 2 actions), TRACE_CALLS launches each
of srlx_vppo_act (k_vppo_act), of srlx_vppo_forward without v (k_vppo_forward: the code the acting launch replaces, before the torch sampling it also removes),
and of the store's push and sample at E = 1024, B = 64; a kernel trace of it gives their times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_distributed_rl_amd.base.run.callback import RunCallback  # noqa: E402

LANES = (16, 64, 1024)
ROUND, SEGMENT, PHASE_STEPS, TRACE_CALLS = 200, 400, 100, 200


def _runner():
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo_v

    runner = srl.Runner("CartPole-v1", ppo_v.Config())
    runner.set_device("cuda:0")
    return runner


def _engine(E):
    """An engine on ppo_v.Config() past its warm-up and its first update."""
    import torch

    from simple_distributed_rl_amd.device.vppo_engine import VppoEngine

    runner = _runner()
    eng = VppoEngine(runner.rl_config, E, seed=1, parameter=runner.make_parameter())
    while eng.replay.is_warmup_needed():
        eng.actor_step()
    eng.step(learner_updates=1)
    torch.cuda.synchronize()
    assert eng.train_count == 1
    return eng


def _round(eng):
    import torch

    torch.cuda.synchronize()
    steps0, updates0, t0 = eng.total_env_steps, eng.train_count, time.perf_counter()
    for _ in range(ROUND):
        eng.step(learner_updates=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(env_steps_per_s=(eng.total_env_steps - steps0) / dt, updates_per_s=(eng.train_count - updates0) / dt, ms_per_lock_step=1e3 * dt / ROUND)


class _Segments(RunCallback):
    """on_step_end hook of the plugin arm: three timed segments past the warm-up, `between(k)` after each."""

    def __init__(self, first: int, between):
        self.start, self.between, self.rounds, self.t0 = first, between, [], None

    def on_step_end(self, context, state, **kwargs) -> bool:
        import torch

        n = state.total_step
        if n == self.start:
            torch.cuda.synchronize()
            self.t0, self.c0 = time.perf_counter(), state.train_count
        elif self.t0 is not None and n == self.start + SEGMENT:
            torch.cuda.synchronize()
            dt = time.perf_counter() - self.t0
            self.rounds.append(dict(env_steps_per_s=SEGMENT / dt, updates_per_s=(state.train_count - self.c0) / dt, ms_per_step=1e3 * dt / SEGMENT))
            self.between(len(self.rounds) - 1)
            self.t0, self.start = None, n + 50
        return False


def _mean(rounds, key):
    return sum(r[key] for r in rounds) / len(rounds)


def measure():
    import torch

    engines = {E: _engine(E) for E in LANES}
    rounds = {E: [] for E in LANES}

    def between(k):
        for E, eng in engines.items():
            rounds[E].append(_round(eng))
            print(f"round {k} engine E={E}", rounds[E][-1], flush=True)

    runner = _runner()
    start_steps = runner.rl_config.memory.warmup_size
    hook = _Segments(start_steps + 200, between)
    runner.train(max_steps=start_steps + 200 + 3 * (SEGMENT + 50) + 10, enable_progress=False, callbacks=[hook])
    assert len(hook.rounds) == 3 and runner.trainer.update_path == "srlx", (len(hook.rounds), runner.trainer.update_path)
    out = dict(plugin=dict(what=f"Runner.train() on the plugin path, one environment: three segments of {SEGMENT} steps past the warm-up, one update per step",
                           rounds=hook.rounds, env_steps_per_s=_mean(hook.rounds, "env_steps_per_s"), updates_per_s=_mean(hook.rounds, "updates_per_s")))
    for E, eng in engines.items():
        eng.phase_times = {}
        for _ in range(PHASE_STEPS):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        host = {k: 1e3 * v / PHASE_STEPS for k, v in eng.phase_times.items()}
        eng.phase_times = None
        out[f"engine_E{E}"] = dict(what=f"VppoEngine.step(learner_updates=1) on the device CartPole, {E} lanes: three rounds of {ROUND} lock-steps",
                                   rounds=rounds[E], env_steps_per_s=_mean(rounds[E], "env_steps_per_s"), updates_per_s=_mean(rounds[E], "updates_per_s"),
                                   host_ms_per_call=dict(actor_step=host["actor"], learner_step=host["learner"]),
                                   env_steps_over_plugin=_mean(rounds[E], "env_steps_per_s") / out["plugin"]["env_steps_per_s"],
                                   updates_over_plugin=_mean(rounds[E], "updates_per_s") / out["plugin"]["updates_per_s"])
    return out


def trace_loop():
    import torch

    from simple_distributed_rl_amd.device.vppo import VppoUpdate
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    n, D, B = 1024, 4, 64
    runner = _runner()
    p = runner.make_parameter()
    u = VppoUpdate(p, max_batch=1)
    x = torch.randn(n, D, device="cuda")
    counter = torch.ones(1, dtype=torch.int64, device="cuda")
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    logp = torch.zeros(n, dtype=torch.float32, device="cuda")
    for _ in range(1 + TRACE_CALLS):
        u.act(n, x, 7, counter, 0.1, actions, logp)
    torch.cuda.synchronize()
    for _ in range(1 + TRACE_CALLS):
        u.forward(x, want_v=False)
    torch.cuda.synchronize()
    store = VppoLanes(n, D, 500, 100_000, B, 1000, 0.95)
    store.reset_all(x)
    r, z = torch.ones(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    done = (torch.arange(n, device="cuda") % 16 == 0).to(torch.uint8)  # 64 lanes close at every other lock-step, episodes of one step
    for k in range(1 + TRACE_CALLS):
        store.push(actions, logp, r, z, done if k % 2 == 0 else z, x, bump=counter)
    torch.cuda.synchronize()
    for _ in range(1 + TRACE_CALLS):
        store.sample()
    torch.cuda.synchronize()
    store.check()
    print(f"trace loop: 1 + {TRACE_CALLS} launches each of k_vppo_act and k_vppo_forward (head only) at {n} rows, D {D}, A 2; the store's push at E {n} and sample at B {B}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vppo_engine_probe.json"))
    ap.add_argument("--trace-loop", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        trace_loop()
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__, config="ppo_v.Config() on CartPole-v1: B 64, D 4, A 2, trunk 64-64, value block 64, no policy block, warm-up 1000")
    out.update(measure())
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("env_steps_per_s", "updates_per_s")} for k, v in out.items() if isinstance(v, dict) and "updates_per_s" in v}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
