"""Probe: the SAC-Discrete device engine (device/sacd_engine.py) next to `Runner.train()` on the plugin path, both on sac.Config() and CartPole, past
the random phase and the warm-up.

    python tools/sacd_engine_probe.py --out profiles/sacd_engine_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o a2 --output-format csv -- python tools/sacd_engine_probe.py --trace-loop 2      # a run of its own, no counters
    rocprofv3 --kernel-trace --stats -d DIR -o a16 --output-format csv -- python tools/sacd_engine_probe.py --trace-loop 16

All arms run in ONE process and are interleaved three times.  The plugin arm is ONE `Runner.train()` call (a second call would restart the Worker's
`step_in_training`, and with it the random phase): an `on_step_end` hook times three segments of SEGMENT environment steps after step START_STEPS + 200, and
between them runs one round of every engine arm.  An engine arm is built beforehand and run, untimed, past its random lock-steps, its warm-up and its first
update; a round is ROUND whole `step(learner_updates=1)` calls ending in a device synchronise.  After the timed rounds every engine runs PHASE_STEPS more
lock-steps with `phase_times` on (the engine then synchronises around `actor_step` and `learner_step`): their host milliseconds per call.
The yardstick of the engine is the plugin arm of the same run.
--trace-loop A runs, at 1024 rows of 4 floats through a 64-64-64 policy with A actions, TRACE_CALLS launches each of srlx_sacd_act (k_sacd_act), of
srlx_sacd_forward with logits only (k_sacd_forward: the code the acting launch replaces, before the uniforms' launch and the argmax it also removes) and, for
A = 2, of srlx_sacd_ring_batch at B = 32 (k_sacd_ring_batch); a kernel trace of it gives their times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_distributed_rl_amd.base.run.callback import RunCallback  # noqa: E402

LANES = (16, 64, 1024)
ROUND, SEGMENT, PHASE_STEPS, TRACE_CALLS = 200, 400, 100, 200


def _runner():
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import sac

    runner = srl.Runner("CartPole-v1", sac.Config())
    runner.set_device("cuda:0")
    return runner


def _engine(E):
    """An engine on sac.Config() past its random lock-steps, its warm-up and its first update."""
    import torch

    from simple_distributed_rl_amd.device.sacd_engine import SacdEngine

    runner = _runner()
    eng = SacdEngine(runner.rl_config, E, seed=1, parameter=runner.make_parameter())
    while eng.lock_steps <= eng.random_until or eng.replay.is_warmup_needed():
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
    """on_step_end hook of the plugin arm: three timed segments past the random phase, `between(k)` after each."""

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
    start_steps = runner.rl_config.start_steps
    hook = _Segments(start_steps + 200, between)
    runner.train(max_steps=start_steps + 200 + 3 * (SEGMENT + 50) + 10, enable_progress=False, callbacks=[hook])
    assert len(hook.rounds) == 3 and runner.trainer.update_path == "srlx", (len(hook.rounds), runner.trainer.update_path)
    out = dict(plugin=dict(what=f"Runner.train() on the plugin path, one environment: three segments of {SEGMENT} steps past start_steps, one update per step",
                           rounds=hook.rounds, env_steps_per_s=_mean(hook.rounds, "env_steps_per_s"), updates_per_s=_mean(hook.rounds, "updates_per_s")))
    for E, eng in engines.items():
        eng.phase_times = {}
        for _ in range(PHASE_STEPS):
            eng.step(learner_updates=1)
        torch.cuda.synchronize()
        host = {k: 1e3 * v / PHASE_STEPS for k, v in eng.phase_times.items()}
        eng.phase_times = None
        out[f"engine_E{E}"] = dict(what=f"SacdEngine.step(learner_updates=1) on the device CartPole, {E} lanes: three rounds of {ROUND} lock-steps",
                                   rounds=rounds[E], env_steps_per_s=_mean(rounds[E], "env_steps_per_s"), updates_per_s=_mean(rounds[E], "updates_per_s"),
                                   host_ms_per_call=dict(actor_step=host["actor"], learner_step=host["learner"]),
                                   env_steps_over_plugin=_mean(rounds[E], "env_steps_per_s") / out["plugin"]["env_steps_per_s"],
                                   updates_over_plugin=_mean(rounds[E], "updates_per_s") / out["plugin"]["updates_per_s"])
    return out


def trace_loop(A: int):
    import sacd_cases as C
    import torch

    from simple_distributed_rl_amd.device import sacd

    n, D = 1024, 4
    p = C.make_parameter(C.make_config(D, A, (64, 64, 64), (128, 128, 128), device="cuda"), 1)
    u = sacd.SacdUpdate(p, max_batch=1)
    x = torch.randn(n, D, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda") * D
    counter = torch.ones(1, dtype=torch.int64, device="cuda")
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(1 + TRACE_CALLS):
        u.act(n, x, off, 7, counter, 0, actions)
    torch.cuda.synchronize()
    for _ in range(1 + TRACE_CALLS):
        u.forward(x, want_q=False)
    torch.cuda.synchronize()
    if A == 2:
        B = 32
        o2 = torch.randint(0, n - 1, (B, 2), device="cuda") * D
        a = torch.zeros(B, dtype=torch.int32, device="cuda")
        r, t = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        s, s2, oh, dn = torch.zeros(B, D, device="cuda"), torch.zeros(B, D, device="cuda"), torch.zeros(B, A, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
        for _ in range(1 + TRACE_CALLS):
            sacd.ring_batch(B, D, A, x, o2, a, r, t, s, s2, oh, dn)
        torch.cuda.synchronize()
    print(f"trace loop: 1 + {TRACE_CALLS} launches each of k_sacd_act and k_sacd_forward (logits only) at {n} rows, D {D}, A {A}, policy 64-64-64")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sacd_engine_probe.json"))
    ap.add_argument("--trace-loop", type=int, default=0, metavar="A")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    if args.trace_loop:
        trace_loop(args.trace_loop)
        return
    t0 = time.time()
    from simple_distributed_rl_amd import _native as N

    out = dict(device=N.device_info(0), torch=torch.__version__, config="sac.Config() on CartPole-v1: B 32, D 4, A 2, policy 64-64-64, q 128-128-128")
    out.update(measure())
    out["wall_s"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {q: v[q] for q in ("env_steps_per_s", "updates_per_s")} for k, v in out.items() if isinstance(v, dict) and "updates_per_s" in v}))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
