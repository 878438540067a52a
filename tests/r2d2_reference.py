"""Float64 yardstick of the R2D2 plugin (simple_distributed_rl_amd/algorithms/r2d2.py, libsrlx srlx_r2d2_seq_td), written from
srl/algorithms/r2d2/r2d2.py by line number as a different program from the code under test.  The reference itself is TensorFlow and is not installed, so
parity with it is UNPINNED: this file is what the tests compare against, and tests/test_r2d2_cpu.py checks its footing with known answers.

  seq_td          r2d2.py:152-209: per-item Python loops on Python floats, as the reference has them; loss and d loss / d q through torch.float64 autograd
                  and torch's own Huber loss (Keras' Huber with delta 1 and mean reduction, :87,209).
  train_step      r2d2.py:109-215 around it: float64 copies of the two networks, burn-in, target pass, online pass, autograd for every parameter's gradient.
  WindowModel     r2d2.py:227-367, the worker's list shifting, as slices of one padded per-episode timeline instead of lists that are popped and appended.
  Walk            a 3-action environment on a flat observation with an invalid action and a time limit, for the trainer-level tests.
  worker_case     seeded episodes of the plugin's Worker on CPU parameters, every call it makes recorded."""
import copy
import math
import random
import types

import numpy as np
import torch

TRAINER_SEEDS = (11, 12)  # the seeds of the trainer-level comparison (tests/test_r2d2_gpu.py) and of its gap condition (tests/test_r2d2_cpu.py)
TRAINER_EPISODES = 3
GAP = 1e-3  # every decision row's top-two gap, as a fraction of max|q|


# ---- r2d2.py:152-209 --------------------------------------------------------------------------------------------------------------------------------------
def rescaling(x, eps=0.001):  # srl/rl/functions.py:10-11
    return math.copysign(1.0, x) * (math.sqrt(abs(x) + 1.0) - 1.0) + eps * x if x != 0 else 0.0


def inverse_rescaling(x, eps=0.001):  # :14-17
    if x == 0:
        return 0.0
    n = (math.sqrt(1.0 + 4.0 * eps * (abs(x) + 1.0 + eps)) - 1.0) / (2.0 * eps)
    return math.copysign(1.0, x) * (n * n - 1.0)


def greedy_probs(q_row, invalid):
    """funcs.calc_epsilon_greedy_probs(q, invalid, 0.0, A) (srl/rl/functions.py:197-214): 1 / (number of maxima among the valid actions) on a maximum."""
    valid = [a for a in range(len(q_row)) if a not in invalid]
    top = max(q_row[a] for a in valid)
    winners = [a for a in valid if q_row[a] == top]
    return [1.0 / len(winners) if a in winners else 0.0 for a in range(len(q_row))]


def targets(frozen_q, q_target, items, discount, retrace_h, enable_retrace, enable_double_dqn, enable_rescale):
    """r2d2.py:153-205.  frozen_q / q_target: float64 [B][S+1][A] arrays; items: dicts with the reference's keys.  Returns (target [B][S], td_mean [B])."""
    S = len(items[0]["actions"])
    target_q_list, td_errors_list = [], []
    for idx, b in enumerate(items):
        retrace, next_td_error, td_errors, target_q = 1.0, 0.0, [], []
        for t in reversed(range(S)):  # :161
            action, mu_prob, reward, done = int(b["actions"][t]), float(b["probs"][t]), float(b["rewards"][t]), bool(b["dones"][t])
            invalid_actions, next_invalid_actions = b["invalid_actions"][t], b["invalid_actions"][t + 1]
            if done:  # :169-170
                gain = reward
            else:
                n_q = frozen_q[idx][t + 1] if enable_double_dqn else q_target[idx][t + 1]  # :173-176
                n_q = [(-math.inf if a in next_invalid_actions else float(v)) for a, v in enumerate(n_q)]  # :177
                n_act_idx = n_q.index(max(n_q))  # :178, np.argmax: the first maximum
                maxq = float(q_target[idx][t + 1][n_act_idx])  # :179
                if enable_rescale:
                    maxq = inverse_rescaling(maxq)  # :181
                gain = reward + discount * maxq  # :182
            if enable_rescale:
                gain = rescaling(gain)  # :184
            target_q.insert(0, gain + retrace * next_td_error)  # :185
            td_error = gain - float(frozen_q[idx][t][action])  # :187
            td_errors.append(td_error)
            if enable_retrace:  # :189-202
                next_td_error = td_error
                pi_prob = greedy_probs([float(v) for v in frozen_q[idx][t]], invalid_actions)[action]
                retrace *= discount * (retrace_h * min(1.0, pi_prob / mu_prob))
        target_q_list.append(target_q)
        td_errors_list.append(sum(td_errors) / len(td_errors))  # :204
    return np.asarray(target_q_list, dtype=np.float64), np.asarray(td_errors_list, dtype=np.float64)


def seq_td(q, q_target, items, weights, discount, retrace_h, enable_retrace, enable_double_dqn, enable_rescale):
    """:146-209 after the forwards.  q: float64 [B][S+1][A] tensor or array.  Returns a namespace: target [B][S], td_mean [B], loss (float), grad_q
    [B][S+1][A] = d loss / d q by autograd (the last step's rows come out zero because :150 drops them)."""
    q = torch.as_tensor(np.asarray(q), dtype=torch.float64).clone().requires_grad_(True)
    qt = np.asarray(q_target, dtype=np.float64)
    target, td_mean = targets(q.detach().numpy(), qt, items, discount, retrace_h, enable_retrace, enable_double_dqn, enable_rescale)
    loss = weighted_huber(q, items, target, weights)
    (grad,) = torch.autograd.grad(loss, q)
    return types.SimpleNamespace(target=target, td_mean=td_mean, loss=float(loss.detach()), grad_q=grad.numpy())


def weighted_huber(q, items, target, weights):
    """:150,208-209: the selected Q of the first S steps against the targets, both times the importance weight, Keras' Huber (delta 1, mean over B * S)."""
    actions = torch.as_tensor(np.asarray([b["actions"] for b in items], dtype=np.int64))
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64)).reshape(-1, 1)
    q_onehot = (q[:, :-1] * torch.nn.functional.one_hot(actions, q.shape[2]).to(torch.float64)).sum(2)
    return torch.nn.functional.huber_loss(q_onehot * w, torch.as_tensor(target) * w, reduction="mean", delta=1.0)


def items_from_arrays(actions, mu, rewards, dones, invalid):
    """Kernel-shaped arrays ([B][S] and the u8 mask [B][S+1][A] or None) -> the reference's item dicts."""
    B, S = actions.shape
    inv = (lambda b, t: [int(a) for a in np.nonzero(invalid[b, t])[0]]) if invalid is not None else (lambda b, t: [])
    return [dict(actions=[int(a) for a in actions[b]], probs=[float(p) for p in mu[b]], rewards=[float(r) for r in rewards[b]],
                 dones=[bool(d) for d in dones[b]], invalid_actions=[inv(b, t) for t in range(S + 1)]) for b in range(B)]


# ---- r2d2.py:109-215 --------------------------------------------------------------------------------------------------------------------------------------
def double_copy(net):
    """A float64 CPU copy of a plugin QNetwork; on CPU tensors its recurrent layer is nn.LSTM itself."""
    return copy.deepcopy(net).to("cpu").double()


def train_step(online64, target64, items, weights, config):
    """One `_train_on_batches` (:109-215) up to the gradients, in float64.  Returns loss, td_mean [B], target [B][S], grads {name: array}, and the
    frozen online / target Q-values [B][S+1][A] (for `decision_gap`)."""
    c = config
    f64 = lambda rows: torch.as_tensor(np.asarray(rows, dtype=np.float64))  # noqa: E731
    burnin_states = f64([[s for s in b["states"][: c.burnin]] for b in items])  # :115
    step_states = f64([[s for s in b["states"][c.burnin :]] for b in items])  # :116
    hidden = (f64([b["hidden_states"][0] for b in items]).unsqueeze(0), f64([b["hidden_states"][1] for b in items]).unsqueeze(0))  # :125-130
    hidden_t = hidden
    online64.train()
    target64.eval()
    with torch.no_grad():
        if c.burnin > 0:  # :134-136
            _, hidden = online64(burnin_states, hidden)
            _, hidden_t = target64(burnin_states, hidden_t)
        q_target, _ = target64(step_states, hidden_t)  # :139
    online64.zero_grad()
    q, _ = online64(step_states, hidden)  # :145
    target, td_mean = targets(q.detach().numpy(), q_target.numpy(), items, c.discount, c.retrace_h, c.enable_retrace, c.enable_double_dqn, c.enable_rescale)
    loss = weighted_huber(q, items, target, weights)
    loss.backward()  # :212
    grads = {k: p.grad.detach().numpy().copy() for k, p in online64.named_parameters()}
    return types.SimpleNamespace(loss=float(loss.detach()), td_mean=td_mean, target=target, grads=grads, q=q.detach().numpy(), q_target=q_target.numpy())


def decision_gap(out, items, enable_double_dqn):
    """The smallest top-two gap, relative to max|q|, over every row an argmax or a maximum is taken of: the selecting rows t + 1 (online under double DQN,
    else target; invalid actions left out, :173-178) and the policy rows t of the online network (:194-199).  A row with one valid action has no gap."""
    S = len(items[0]["actions"])
    scale = max(float(np.abs(out.q).max()), float(np.abs(out.q_target).max()))
    gaps = []
    for idx, b in enumerate(items):
        for t in range(S):
            for row, invalid in (((out.q if enable_double_dqn else out.q_target)[idx][t + 1], b["invalid_actions"][t + 1]), (out.q[idx][t], b["invalid_actions"][t])):
                v = sorted((float(x) for a, x in enumerate(row) if a not in invalid), reverse=True)
                if len(v) > 1:
                    gaps.append(v[0] - v[1])
    return min(gaps) / scale


# ---- r2d2.py:227-367 --------------------------------------------------------------------------------------------------------------------------------------
class WindowModel:
    """The items one episode hands to the memory, from the episode's record.  Every per-step list of the worker is a window of fixed length sliding over one
    timeline: [what on_reset pads with] + [the episode] + [what the flush after `done` pads with]; after n shifts the window starts at entry n.

    record: s (T + 1 states), a / prob / reward / terminated (T each), invalid (T + 1 lists: before every step and after the last), hidden (T + 1 pairs
    [h, c]: the zero state, then the state after each policy call), q_taken (T: q[a] of each policy call), done (whether the last step ended the episode),
    pads_reset (sequence_length random actions, :237), pads_flush (one random action per flushed item, :317)."""

    def __init__(self, burnin, sequence_length, n_actions, discount, enable_rescale):
        self.burnin, self.S, self.A, self.discount, self.rescale = burnin, sequence_length, n_actions, discount, enable_rescale
        self.L = burnin + sequence_length + 1

    def items(self, rec):
        S, L, T = self.S, self.L, len(rec.a)
        n_flush = S - 1 if rec.done else 0  # :313 `len(recent_rewards) - 1`
        assert len(rec.pads_reset) == S and len(rec.pads_flush) == n_flush
        dummy = np.zeros_like(np.asarray(rec.s[0], dtype=np.float32))
        states = [dummy] * (L - 1) + [np.asarray(s, dtype=np.float32) for s in rec.s] + [dummy] * n_flush  # :236,246-247,282,315
        actions = list(rec.pads_reset) + list(rec.a) + list(rec.pads_flush)  # :237,284,317
        probs = [1.0 / self.A] * S + list(rec.prob) + [1.0 / self.A] * n_flush  # :238,286,319
        rewards = [0.0] * S + list(rec.reward) + [0.0] * n_flush  # :239,288,321
        dones = [False] * S + list(rec.terminated) + [True] * n_flush  # :240,290,323
        invalid = [[] for _ in range(S)] + list(rec.invalid) + [[] for _ in range(n_flush)]  # :241,248-249,292,325
        hidden = [rec.hidden[0]] * (L - 1) + list(rec.hidden)  # :244,293-299; the flush only pops (:326), so the head keeps walking this timeline
        out = []
        for n in range(1, T + n_flush + 1):  # the window after n shifts
            out.append(dict(states=states[n : n + L], actions=actions[n : n + S], probs=probs[n : n + S], rewards=rewards[n : n + S], dones=dones[n : n + S],
                            invalid_actions=invalid[n : n + S + 1], hidden_states=hidden[n]))
        return out

    def adds(self, rec, distributed_priorities):
        """The (item, priority) pairs in the order `memory.add` receives them.  Without priorities: every item once, priority None (:367).  With them
        (:335-349): nothing until the flush, then after EVERY flushed item the whole history so far, newest first, with its Monte-Carlo priority."""
        items = self.items(rec)
        if not distributed_priorities:
            return [(it, None) for it in items]
        T = len(rec.a)
        info = [(float(rec.q_taken[n]), float(rec.reward[n])) for n in range(T)] + [(float(rec.q_taken[T - 1]), 0.0)] * (len(items) - T)  # :302-305,329-332
        out = []
        for upto in range(T + 1, len(items) + 1):
            ret = 0.0
            for n in reversed(range(upto)):
                ret = info[n][1] + self.discount * (inverse_rescaling(ret) if self.rescale else ret)  # :340-344
                if self.rescale:
                    ret = rescaling(ret)
                out.append((items[n], abs(ret - info[n][0])))  # :348-349
        return out


# ---- the trainer-level case: a 3-action walk and the plugin's Worker on CPU parameters ------------------------------------------------------------------
def register_walk():
    from simple_distributed_rl_amd.base.define import SpaceTypes
    from simple_distributed_rl_amd.base.env import registration
    from simple_distributed_rl_amd.base.env.base import EnvBase
    from simple_distributed_rl_amd.base.spaces.box import BoxSpace
    from simple_distributed_rl_amd.base.spaces.discrete import DiscreteSpace

    global Walk
    if "Walk" in globals():
        return

    class Walk(EnvBase):
        """Cells 0..5, start at 1; actions left / stay / right, left invalid in cell 0; -0.05 per step, +1 and the end in cell 5; 9 steps at the most (the
        time limit ends an episode without `terminated`).  The observation is flat: (cell / 5, step / 9)."""

        def __init__(self):
            super().__init__()
            self.pos, self.t = 1, 0

        action_space = property(lambda self: DiscreteSpace(3))
        observation_space = property(lambda self: BoxSpace((2,), 0, 1, np.float32, SpaceTypes.CONTINUOUS))
        max_episode_steps = property(lambda self: 9)
        player_num = property(lambda self: 1)

        def _obs(self):
            return np.array([self.pos / 5, self.t / 9], dtype=np.float32)

        def reset(self, *, seed=None, **kwargs):
            self.pos, self.t = 1, 0
            return self._obs()

        def step(self, action):
            self.pos = min(max(self.pos + int(action) - 1, 0), 5)
            self.t += 1
            return self._obs(), (1.0 if self.pos == 5 else -0.05), self.pos == 5, False

        def get_invalid_actions(self, player_index=-1):
            return [0] if self.pos == 0 else []

        def backup(self, **kwargs):
            return (self.pos, self.t)

        def restore(self, data, **kwargs):
            self.pos, self.t = data

    registration.register("R2D2Walk-v0", __name__ + ":Walk", check_duplicate=False)


def small_config(retrace=True, **kw):
    """The trainer-level tests' configuration: B 4, burnin 2, sequence_length 3, lstm_units 16, dueling (32,)."""
    from simple_distributed_rl_amd.algorithms import r2d2

    c = r2d2.Config(batch_size=4, burnin=2, sequence_length=3, lstm_units=16, enable_retrace=retrace, epsilon=0.5, **kw)
    c.hidden_block.set_dueling_network((32,))
    c.memory.capacity, c.memory.warmup_size = 256, 4
    return c


class _RandintLog:
    """Stands in for the `random` module inside algorithms/r2d2.py: every randint the worker draws (its pad actions) is recorded."""

    def __init__(self):
        self.draws = []

    def randint(self, a, b):
        self.draws.append(random.randint(a, b))
        return self.draws[-1]


def worker_case(config, env_id, seed, episodes, distributed=False):
    """Plays `episodes` seeded episodes with the plugin's Worker on CPU parameters and a recording memory.  Returns (records, adds, parameter): one record per
    episode in WindowModel's form, and every (item, priority) the worker handed to `memory.add`, in order."""
    import simple_distributed_rl_amd as srl
    from simple_distributed_rl_amd.algorithms import r2d2
    from simple_distributed_rl_amd.base.rl.worker_run import WorkerRun

    records, adds, log = [], [], _RandintLog()

    class RecordingWorker(r2d2.Worker):
        distributed = property(lambda self: distributed)

        def on_reset(self, worker):
            n0 = len(log.draws)
            super().on_reset(worker)
            h0 = self.parameter.convert_numpy_from_hidden_state(self.hidden_state)
            records.append(types.SimpleNamespace(s=[worker.state.astype(np.float32)], a=[], prob=[], reward=[], terminated=[], invalid=[list(worker.invalid_actions)],
                                                 hidden=[h0], q_taken=[], done=False, pads_reset=log.draws[n0:], pads_flush=[]))

        def policy(self, worker):
            a = super().policy(worker)
            r = records[-1]
            r.a.append(a)
            r.prob.append(self.prob)
            r.q_taken.append(self.q[a])
            r.hidden.append(self.parameter.convert_numpy_from_hidden_state(self.hidden_state))
            return a

        def on_step(self, worker):
            r, n0 = records[-1], len(log.draws)
            r.s.append(worker.next_state.astype(np.float32))
            r.reward.append(worker.reward)
            r.terminated.append(worker.terminated)
            r.invalid.append(list(worker.next_invalid_actions))
            r.done = bool(worker.done)
            super().on_step(worker)
            r.pads_flush = log.draws[n0:]

    class RecordingMemory:
        def add(self, batch, priority=None, serialized=False):
            adds.append((batch, priority))

        def length(self):
            return len(adds)

    torch.manual_seed(seed)
    r = srl.Runner(env_id, config)
    r.set_device("CPU")
    r.set_seed(seed)
    parameter = r.make_parameter()
    real_random, r2d2.random = r2d2.random, log
    try:
        r._memory = RecordingMemory()
        r._worker = WorkerRun(RecordingWorker(r.rl_config, parameter, r._memory), r.make_env())
        r.rollout(max_episodes=episodes)
    finally:
        r2d2.random = real_random
    return records, adds, parameter
