"""GPU tests of the E-environment Agent57_light engine (BASELINE.json configs[3] workload; reference:
srl/algorithms/agent57_light/agent57_light.py:271-471, model_torch.py:263-443)."""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

import simple_distributed_rl_amd as srl  # noqa: E402
from simple_distributed_rl_amd.algorithms import agent57_light  # noqa: E402


def test_ucb_bank_equals_the_host_controller_per_environment():
    """srlx_agent57_ucb_step vs UcbMetaController (pinned to the reference's trace in tests/test_agent57_cpu.py): E controllers, each
    fed its own episode rewards; the host controller gets the SAME uniforms through a patched `random` (epsilon draw, random arm)."""
    from agent57_kernels_reference import HostUcbBank
    from simple_distributed_rl_amd.device.agent57_light import UcbBank

    E, Na, window, eps, beta = 5, 4, 9, 0.2, 0.7
    dev = torch.device("cuda:0")
    bank = UcbBank(E, Na, window, eps, beta, dev, seed=1)
    rng = np.random.default_rng(0)

    hosts = HostUcbBank(E, Na, window, eps, beta)  # the Feed / tie_break arrangement: tests/agent57_kernels_reference.py
    got_rows, want_rows = [], []
    last = np.zeros(E, np.float32)
    for it in range(60):
        done = (rng.random(E) < 0.7).astype(np.uint8) if it > 0 else np.ones(E, np.uint8)
        u = rng.random((E, 3))
        arms = bank.step(torch.as_tensor(done, device=dev), torch.as_tensor(last, device=dev), torch.as_tensor(u, device=dev)).cpu().numpy().copy()
        got_rows.append(arms)
        want_rows.append(hosts.step(done, last, u))
        last = rng.integers(-3, 4, E).astype(np.float32)  # small integers: ties between arms do occur
    np.testing.assert_array_equal(np.array(got_rows), np.array(want_rows))
    assert int(bank.n_recent.max()) == window - 1  # the window slid


def _engine(E=8, intrinsic=True, capacity=8 * 40, warmup=32, batch=8, episode_len=9):
    from simple_distributed_rl_amd.device.agent57_light import Agent57LightEngine

    cfg = agent57_light.Config(batch_size=batch, actor_num=4, enable_intrinsic_reward=intrinsic, target_model_update_interval=5, episodic_memory_capacity=64,
                               ucb_window_size=6)
    cfg.window_length = 4
    cfg.memory.capacity, cfg.memory.warmup_size = capacity, warmup
    cfg.memory.set_proportional(alpha=0.6, beta_initial=0.4, beta_steps=1000)
    cfg.input_block.image.set_dqn_block()
    cfg.hidden_block.set_dueling_network((32,))
    env = srl.make_env(srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(hw=(20, 20), n_actions=3, episode_len=episode_len)))
    cfg.setup(env)
    return Agent57LightEngine(cfg, E, 0, episode_len=episode_len, seed=3), cfg


def test_engine_items_are_consistent_and_the_learner_trains():
    eng, cfg = _engine()
    E, L = eng.E, eng.L
    hist = []
    for t in range(30):
        slot = eng.replay._steps_committed % L
        pa, arm, reset = eng.prev_action.clone(), eng.arm().clone(), eng.reset_lane.clone()
        eng.step(learner_updates=1)
        hist.append((slot, pa.cpu().numpy(), arm.cpu().numpy(), eng.actions.cpu().numpy().copy(), reset.cpu().numpy(), eng.x_r_int[slot].cpu().numpy().copy(),
                     eng.env.done.cpu().numpy().copy()))
    torch.cuda.synchronize()
    assert eng.train_count > 10 and all(np.isfinite(v) for v in eng.learner.losses().values())
    # what was written per slot is what the lanes held when they acted; previous action chains through live lanes; arms change only at episode ends
    for t in range(1, 30):
        slot, pa, arm, act, reset, r_int, done = hist[t]
        _, _, arm_prev, act_prev, reset_prev, _, done_prev = hist[t - 1]
        live_prev = reset_prev == 0
        np.testing.assert_array_equal(eng.x_prev_action[slot].cpu().numpy(), pa)  # (L = 45 slots > 30 lock-steps: nothing overwritten yet)
        np.testing.assert_array_equal(eng.x_actor[slot].cpu().numpy(), arm)
        keep = live_prev & (done_prev == 0)
        np.testing.assert_array_equal(pa[keep], act_prev[keep])  # previous action = the action of the previous live lock-step
        np.testing.assert_array_equal(arm[done_prev == 0], arm_prev[done_prev == 0])  # an arm lasts an episode
        assert (r_int[reset == 1] == 0).all() and (r_int[reset == 0] >= 0).all()
        if cfg.enable_intrinsic_reward and (reset == 0).any():  # (the synthetic lanes end their episodes together: some lock-steps are all resets)
            assert (r_int[reset == 0] > 0).any()
    assert int(eng.ucb.arm.min()) >= 0 and int(eng.ucb.arm.max()) < cfg.actor_num
    # sampled items gather exactly those fields
    b = eng.replay.batch
    e, s = eng.loc_env.cpu().numpy(), eng.loc_slot.cpu().numpy()
    assert ((0 <= e) & (e < E)).all() and ((0 <= s) & (s < L)).all()
    assert eng.info()["memory"] > 0


def test_engine_without_intrinsic_reward_and_evaluation_mode():
    eng, cfg = _engine(intrinsic=False)
    for _ in range(12):
        eng.step(learner_updates=1)
    assert float(eng.x_r_int.abs().max()) == 0.0 and eng.train_count > 0
    eng.training = False  # test_epsilon / test_beta, arm 0 (agent57_light.py:294-297)
    q_ext, q_int, q = eng.policy_q()
    torch.testing.assert_close(q, q_ext + cfg.test_beta * q_int)


def test_bench_agent57_light_line():
    """`bench.py --algo agent57_light` prints the contract's JSON line for the configs[3] workload on one GPU."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--algo", "agent57_light", "--envs", "64", "--capacity", "20000", "--steps", "2", "--inner", "4",
                        "--warmup", "1", "--no-cpu-baseline", "--no-per-micro", "--no-subfigures"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and "Agent57_light" in d["config"]["workload"] and d["value"] > 0 and d["learner_updates_per_s"] > 0
    assert d["final"]["train_count"] >= 2 * 4


def test_runner_train_and_train_mp_with_agent57_light():
    """`srl.Runner(env, agent57_light.Config()).train()` / `.train_mp()` on GPU devices reach the E-environment engine and the one-process-
    per-rank topology (BASELINE.json configs[3]; here 2 ranks time-sharing the test GPU over gloo)."""
    cfg = agent57_light.Config(batch_size=8, actor_num=4, target_model_update_interval=5, episodic_memory_capacity=64, ucb_window_size=6)
    cfg.window_length = 4
    cfg.memory.capacity, cfg.memory.warmup_size = 2 * 8 * 30, 32
    cfg.memory.set_proportional(alpha=0.6, beta_initial=0.4, beta_steps=1000)
    cfg.hidden_block.set_dueling_network((32,))
    runner = srl.Runner(srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(hw=(20, 20), n_actions=3, episode_len=7)), cfg)
    runner.set_vector_envs(8)
    before = {k: v.detach().clone() for k, v in runner.parameter.q_ext_online.state_dict().items()}
    st = runner.train(max_train_count=10, train_interval=8)
    assert runner.vector_reason == "" and st.end_reason == "max_train_count over." and st.train_count >= 10
    assert st.episode_count > 0 and st.memory.length() > 32
    after = runner.parameter.q_ext_online.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)  # the Runner's own parameter object was trained
    st = runner.train_mp(actor_num=2, actor_devices=["cuda:0", "cuda:0"], max_train_count=12, timeout=300, sync_interval_steps=4)
    assert runner.vector_reason == "" and st.end_reason == "max_train_count over." and st.train_count >= 12 and st.trainer_recv_q > 0


@pytest.mark.parametrize("hw", [84, 20])
def test_image_trunks_equal_the_torch_image_blocks(hw):
    """device/qnet.py:ImageTrunk (libsrlx convolutions straight from the uint8 ring, the module's own weights bound by address) vs the
    torch image block on the float32 stack of the same frames, for the engine's five networks -- and the actor's Q-values / intrinsic
    reward inputs built from them (84 x 84: the fused kernel; 20 x 20: the three-launch path)."""
    from simple_distributed_rl_amd.device.agent57_light import Agent57LightEngine, embed, q_values, rnd

    cfg = agent57_light.Config(batch_size=8, actor_num=4, target_model_update_interval=5, episodic_memory_capacity=64, ucb_window_size=6)
    cfg.window_length = 4
    cfg.memory.capacity, cfg.memory.warmup_size = 8 * 40, 32
    cfg.memory.set_proportional(alpha=0.6, beta_initial=0.4, beta_steps=1000)
    cfg.input_block.image.set_dqn_block()
    cfg.hidden_block.set_dueling_network((32,))
    env = srl.make_env(srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(hw=(hw, hw), n_actions=3, episode_len=9)))
    cfg.setup(env)
    eng = Agent57LightEngine(cfg, 8, 0, episode_len=9, seed=3)
    assert eng._all_fused and set(eng._trunks) == {"q_ext", "q_int", "emb", "rnd_target", "rnd_train"}
    p = eng.parameter
    for it in range(14):
        eng.step(learner_updates=1)  # the weights move: the trunks must follow them
        stack = eng.replay.stack_current().view(eng.E, eng.Wn, *eng.hw)
        off = eng.replay.frame_table_current()
        nets = {"q_ext": p.q_ext_online, "q_int": p.q_int_online, "emb": p.emb_network, "rnd_target": p.lifelong_target, "rnd_train": p.lifelong_train}
        with torch.no_grad():
            for name, net in nets.items():
                want = net.in_block(stack, channels_first=True)
                got = eng._trunks[name](eng.replay.obs_base, off)
                torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * float(want.abs().max()), msg=lambda m, n=name: f"{n} (iteration {it}): {m}")
            arm = eng.arm()
            inputs = (stack, eng.prev_r_ext.view(-1, 1), eng.prev_r_int.view(-1, 1), eng.action_eye[eng.prev_action], eng.actor_eye[arm])
            q_ext, q_int, _ = eng.policy_q()
            torch.testing.assert_close(q_ext, q_values(p.q_ext_online, *inputs), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(q_int, q_values(p.q_int_online, *inputs), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(embed(p.emb_network, None, eng._trunks["emb"](eng.replay.obs_base, off)), embed(p.emb_network, stack), rtol=1e-4, atol=1e-5)
            torch.testing.assert_close(rnd(p.lifelong_train, None, eng._trunks["rnd_train"](eng.replay.obs_base, off)), rnd(p.lifelong_train, stack), rtol=1e-4, atol=1e-5)
    assert eng.train_count > 5


def _engine84(batch=16, E=16, seed=3, torch_learner=False):
    from simple_distributed_rl_amd.device.agent57_light import Agent57LightEngine

    cfg = agent57_light.Config(batch_size=batch, actor_num=4, target_model_update_interval=5, episodic_memory_capacity=64, ucb_window_size=6)
    cfg.window_length = 4
    cfg.memory.capacity, cfg.memory.warmup_size = E * 40, 64
    cfg.memory.set_proportional(alpha=0.6, beta_initial=0.4, beta_steps=1000)
    cfg.input_block.image.set_dqn_block()
    cfg.hidden_block.set_dueling_network((64,))
    env = srl.make_env(srl.EnvConfig("SyntheticAtari-v0", kwargs=dict(hw=(84, 84), n_actions=4, episode_len=11)))
    cfg.setup(env)
    return Agent57LightEngine(cfg, E, 0, episode_len=11, seed=seed, torch_learner=torch_learner), cfg


def test_trainable_trunk_gradients_equal_autograd():
    """device/qnet.py:TrainableImageTrunk -- the image block's forward AND backward in libsrlx (srlx_qnet_backward_convs_u8) -- against autograd through the
    SAME torch image block evaluated in float64 on the CPU, on the float32 stack of the same frames: features and all six gradients 1e-5 relative to their
    largest element, with gradient on every row (stride 1) and on every second row only (stride 2: the online Q-network's s_0 / s_1 pass).
    (The yardstick used to be autograd on the GPU, i.e. MIOpen's float32 convolution backward, at 2e-4: in about one fresh process of eight MIOpen's own
    gradients were off by 4e-4 .. 1.4e-2 of their largest element against float64 while libsrlx's stayed at 3e-7 .. 9e-7 -- tools/_flaky_trunk.py.)
    The networks are initialised from torch's global generator: seeded here, because a comparison of ReLU networks across precisions is only as tight as
    its closest-to-zero activation -- about one random initialisation in fifty puts a conv3 output within float32 rounding of zero, the two evaluations
    then disagree on that element's mask and every gradient moves by ~1e-3 of its largest element (reproducibly for that network; features still 3e-7)."""
    import copy

    torch.manual_seed(7)

    eng, cfg = _engine84()
    for _ in range(8):
        eng.step(learner_updates=0)
    assert eng._ltrunks is not None and set(eng._ltrunks) == {"q_ext", "q_ext_t", "q_int", "q_int_t", "emb", "ll", "ll_t"}
    rp = eng.replay
    rp.sample_items(eng.train_count_dev, all_states=True)
    B, W = rp.B, eng.Wn
    off01 = rp.frame_off_all.view(2 * B, W)
    b = rp.sample(eng.train_count_dev.clone())  # the float32 windows of a second draw are not the same items: gather the drawn ones instead
    N_ = rp.lib
    from simple_distributed_rl_amd import _native as N

    obs = torch.zeros((B, 2, W, 84 * 84), dtype=torch.float32, device="cuda")
    rp.sample_items(eng.train_count_dev, all_states=True)
    N.check(N_.srlx_store_gather_nstep(rp.h_store, B, N.tptr(rp.batch.indices), N.tptr(obs), N.tptr(rp.batch.actions), N.tptr(rp.batch.rewards), N.tptr(rp.batch.terminated),
                                       N.torch_stream_ptr()))
    stack = obs.view(2 * B, W, 84, 84)
    net = eng.parameter.emb_network
    trunk = eng._ltrunks["emb"]
    params = [t for c in trunk.convs for t in (c.weight, c.bias)]
    g = torch.Generator(device="cuda").manual_seed(5)
    for stride in (1, 2):
        R = torch.randn((2 * B, trunk.channels * trunk.pixels), device="cuda", generator=g)
        if stride == 2:
            R[1::2] = 0  # rows without gradient
        blk64 = copy.deepcopy(net.in_block).double().cpu()
        for q in blk64.parameters():
            q.grad = None
        want_f = blk64(stack.double().cpu(), channels_first=True)
        (want_f * R.double().cpu()).sum().backward()
        want = [t for c in [m for m in blk64.modules() if isinstance(m, torch.nn.Conv2d)] for t in (c.weight.grad, c.bias.grad)]
        assert len(want) == len(params) and all(w.shape == p.shape for w, p in zip(want, params))
        for p in params:
            p.grad = None
        got_f = trunk.features(rp.obs_base, off01, stride)
        torch.testing.assert_close(got_f.double().cpu(), want_f.detach(), rtol=1e-5, atol=1e-5 * float(want_f.abs().max()))
        (got_f * R).sum().backward()
        for p, w in zip(params, want):
            torch.testing.assert_close(p.grad.double().cpu(), w, rtol=1e-5, atol=1e-5 * float(w.abs().max()))


def test_hand_written_learner_matches_the_torch_learner_argument_and_is_reproducible():
    """The update with the image blocks of all five networks in libsrlx (forward + backward; no MIOpen on the update path) against the same update through
    torch's convolutions (torch_learner=True) from the same seed.  Two statements, two tolerances:
    * the FIRST update's four losses -- same weights, same batch, only the forward arithmetic differs (split-bf16 products on the matrix pipe against
      MIOpen's fp32 convolutions) -- agree to north_star's 1e-5;
    * after 12 updates the losses agree to 5e-3 (1e-3 held for the three-part bf16 split of rounds 3-5; round 6's two-part float16 split -- the same 2.9e-7 forward
      error against float64, tools/conv_split_error.py -- lands on another of these trajectories: 2.2e-3 on emb_loss).  That is a statement about two float32 Adam TRAJECTORIES, not about a kernel: Adam divides by
      sqrt(v) + eps, so a parameter whose gradient is a cancellation residue moves by the full learning rate in a direction that the last bits of the
      gradient sum decide; the two learners order their gradient sums differently (MIOpen's solver against ticketed MFMA partials), the differences
      compound over the updates, and MIOpen's own fp32 solvers differ more from each other than 1e-3 over the same 12 updates (round 3: one instance
      in four landed on a different trajectory).  A per-update bound is the first bullet; the single-update gradients are held to 2e-4 of max |g|
      in test_trainable_trunk_gradients_equal_autograd above, the whole update against a recorded Trainer.train() of the reference in tests/test_agent57_cpu.py / test_agent57_gpu.py (golden
      train_step_agent57_light.npz).
    Two hand-written instances give the SAME losses bit for bit."""
    def run(torch_learner):
        torch.manual_seed(11)  # the five networks are initialised from torch's global generator
        random.seed(11)
        np.random.seed(11)
        eng, _ = _engine84(torch_learner=torch_learner)
        assert (eng._ltrunks is None) == torch_learner
        first = None
        for _ in range(20):
            eng.step(learner_updates=1)
            if first is None and eng.train_count == 1:
                torch.cuda.synchronize()
                first = dict(eng.learner.losses())
        torch.cuda.synchronize()
        assert eng.train_count >= 12 and first is not None
        return eng.learner.losses(), eng.train_count, first

    a, na, fa = run(False)
    b, nb, fb = run(False)
    t, nt, ft = run(True)
    assert na == nb == nt and a == b and fa == fb, (a, b)
    for k in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        assert abs(fa[k] - ft[k]) <= 1e-5 * max(abs(ft[k]), 1e-2), ("first update", k, fa[k], ft[k])
    for k in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss"):
        assert math.isfinite(a[k]) and abs(a[k] - t[k]) <= 5e-3 * max(abs(t[k]), 1e-3), (k, a[k], t[k])


def test_overlapped_update_runs_beside_the_actors():
    """Agent57LightEngine(overlap=True): the update (one HIP graph, launched by the helper thread on the learner's stream) beside the actors' lock-step, joined
    before the ring commit; the actors act on private copies of the two Q-networks that equal the online ones after every lock-step; the run trains (finite
    losses, the expected number of updates) and two overlapped instances walk one trajectory."""
    from simple_distributed_rl_amd.device.agent57_light import Agent57LightEngine

    def run():
        torch.manual_seed(0)  # (the networks' initialisation draws from torch's global generator)
        eng, cfg = _engine84(batch=16, E=16, seed=3)
        del eng
        eng = Agent57LightEngine(cfg, 16, 0, episode_len=11, seed=3, overlap=True)
        for k in range(30):
            if k == 12:
                eng.join_learner()
                eng.capture_graphs()
            eng.step(learner_updates=1)
        eng.join_learner()
        torch.cuda.synchronize()
        p = eng.parameter
        for name, src in (("q_ext", p.q_ext_online), ("q_int", p.q_int_online), ("emb", p.emb_network), ("rnd_train", p.lifelong_train)):
            for a, b in zip(eng._act_q[name].parameters(), src.parameters()):
                assert torch.equal(a, b), name
        info = eng.info()
        assert eng.train_count >= 20 and all(np.isfinite(info[k]) for k in ("ext_loss", "int_loss", "emb_loss", "lifelong_loss")), info
        return info, float(sum(float(q.double().sum()) for q in p.q_ext_online.parameters()))

    a, b = run(), run()
    assert a == b
