"""Probe: the V-PPO device engine on the Normal head (device/vppo_engine.py: VppoNormalEngine) next to `Runner.train()` on the plugin path, both on
ppo_v.Config() and Pendulum-v1, past the warm-up.

    python tools/vppo_normal_engine_probe.py --out profiles/vppo_normal_engine_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o act --output-format csv -- python tools/vppo_normal_engine_probe.py --trace-loop    # a run of its own, no counters

The method is tools/vppo_engine_probe.py's, whose helpers this probe uses: all arms in ONE process, interleaved three times; the plugin arm is ONE
`Runner.train()` call timed in three segments by an `on_step_end` hook, with one round of every engine arm between them; an engine arm is built beforehand and run,
untimed, past its warm-up and its first update (on the device Pendulum the first episodes close at lock-step 200, all lanes at once); afterwards every engine runs
PHASE_STEPS lock-steps with `phase_times` on for the host milliseconds of `actor_step` and `learner_step`.  The yardstick is the plugin arm of the same run.
--trace-loop runs, at 1024 rows of 3 floats through ppo_v.Config()'s network (trunk 64-64, value block 64, no policy block, one action element), TRACE_CALLS
launches each of srlx_vppo_act_normal (k_vppo_act_normal), of srlx_vppo_forward without v (k_vppo_forward: the code the acting launch replaces, before the host's
draw it also removes), of srlx_pendulum_lane_step, and of the K = 1 float store's push and sample at E = 1024, B = 64; a kernel trace of it gives their times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vppo_engine_probe import LANES, PHASE_STEPS, ROUND, SEGMENT, TRACE_CALLS, _mean, _round, _Segments  # noqa: E402


def _runner():
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import ppo_v

    runner = srl.Runner("Pendulum-v1", ppo_v.Config())
    runner.set_device("cuda:0")
    return runner


def _engine(E):
    """An engine on ppo_v.Config() past its warm-up and its first update."""
    import torch

    from simple_distributed_rl_amd.device.vppo_engine import VppoNormalEngine

    runner = _runner()
    eng = VppoNormalEngine(runner.rl_config, E, seed=1, parameter=runner.make_parameter())
    while eng.replay.is_warmup_needed():
        eng.actor_step()
    eng.step(learner_updates=1)
    torch.cuda.synchronize()
    assert eng.train_count == 1
    return eng


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
        eng.replay.check()
        out[f"engine_E{E}"] = dict(what=f"VppoNormalEngine.step(learner_updates=1) on the device Pendulum, {E} lanes: three rounds of {ROUND} lock-steps",
                                   rounds=rounds[E], env_steps_per_s=_mean(rounds[E], "env_steps_per_s"), updates_per_s=_mean(rounds[E], "updates_per_s"),
                                   host_ms_per_call=dict(actor_step=host["actor"], learner_step=host["learner"]),
                                   env_steps_over_plugin=_mean(rounds[E], "env_steps_per_s") / out["plugin"]["env_steps_per_s"],
                                   updates_over_plugin=_mean(rounds[E], "updates_per_s") / out["plugin"]["updates_per_s"])
    return out


def trace_loop():
    import torch

    from simple_distributed_rl_amd.device.mlpq import PendulumLaneVecEnv
    from simple_distributed_rl_amd.device.vppo import VppoUpdate
    from simple_distributed_rl_amd.device.vppo_lanes import VppoLanes

    n, D, K, B = 1024, 3, 1, 64
    runner = _runner()
    p = runner.make_parameter()
    u = VppoUpdate(p, max_batch=1)
    x = torch.randn(n, D, device="cuda")
    counter = torch.ones(1, dtype=torch.int64, device="cuda")
    low, high = torch.full((K,), -2.0, device="cuda"), torch.full((K,), 2.0, device="cuda")
    actions, logp, env_actions = (torch.zeros((n, K), dtype=torch.float32, device="cuda") for _ in range(3))
    for _ in range(1 + TRACE_CALLS):
        u.act_normal(n, x, 7, counter, 0.1, 0.5, True, low, high, actions, logp, env_actions)
    torch.cuda.synchronize()
    for _ in range(1 + TRACE_CALLS):
        u.forward(x, want_v=False)
    torch.cuda.synchronize()
    store = VppoLanes(n, D, 500, 100_000, B, 1000, 0.95, action_dim=K)
    store.reset_all(x)
    env = PendulumLaneVecEnv(store, max_steps=200)
    env.reset()
    for _ in range(1 + TRACE_CALLS):
        env.step(env_actions)
    torch.cuda.synchronize()
    r, z = torch.ones(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    done = (torch.arange(n, device="cuda") % 16 == 0).to(torch.uint8)  # 64 lanes close at every other lock-step, episodes of one step
    for k in range(1 + TRACE_CALLS):
        store.push(actions, logp, r, z, done if k % 2 == 0 else z, x, bump=counter)
    torch.cuda.synchronize()
    for _ in range(1 + TRACE_CALLS):
        store.sample()
    torch.cuda.synchronize()
    store.check()
    print(f"trace loop: 1 + {TRACE_CALLS} launches each of k_vppo_act_normal and k_vppo_forward (head only) at {n} rows, D {D}, K {K}; k_pendulum_lanes at E {n}; the "
          f"store's push at E {n} and sample at B {B}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vppo_normal_engine_probe.json"))
    ap.add_argument("--trace-loop", action="store_true")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        trace_loop()
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__,
               config="ppo_v.Config() on Pendulum-v1: B 64, D 3, K 1, squashed, trunk 64-64, value block 64, no policy block, warm-up 1000, episodes of 200 steps")
    out.update(measure())
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("env_steps_per_s", "updates_per_s")} for k, v in out.items() if isinstance(v, dict) and "updates_per_s" in v}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
