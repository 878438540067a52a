"""The yardstick of NoT_SAC's update: a float64 restatement of srl/algorithms/sac_not/torch_model.py:131-191 and of the two distribution blocks it uses
(srl/rl/torch_/distributions/normal_dist_block.py:49-54,121-145, categorical_gumbel_dist_block.py:10-12,45-60), written as a different program from the
plugin and the kernels: the networks are walked layer by layer on float64 copies, the losses and their seeds d loss / d q are explicit per-row formulas in
Python floats, autograd carries the seeds through the networks only, the norm clips and Adam are explicit formulas.  It takes the plugin's `noise`.
tests/test_notsac_pinned_cpu.py holds it to the reference's own code.

Every update reports `margin`, the smallest distance of the update from a kink of the arithmetic: |target - q| against Huber's 1 (relative); a raw log-scale
against either end of the clamp (absolute, in the log domain); the gap between the two largest noisy next-state logits (absolute: the argmax that picks the
one-hot next action); each of the two gradient norms against max_grad_norm (relative).  ReLU and SiLU are continuous and need no margin.  Comparisons of
float32 code against this module only mean something away from the kinks: tests/test_notsac_cpu.py requires 1e-3 of every update of every case."""
import copy
import math

import torch

GUMBEL_EPS = 1e-6


def _chain(block, x):
    for layer in block.hidden_layers:
        x = layer(x)
    return x


def policy_forward(policy, state):
    """The head's raw outputs of a float64 copy of sac_not.PolicyNetwork: logits [B][A], or (locs, RAW log-scales) [B][K] each."""
    h = _chain(policy.policy_block, _chain(policy.in_block, state))
    dist = policy.policy_dist_block
    if hasattr(dist, "loc_layers"):
        return dist.loc_layers[0](h), dist.log_scale_layers[0](h)
    return dist.h_layers[0](h)


def q_forward(qnet, state, action):
    """q [B] of a float64 copy of sac_not.QNetwork, the SiLU written out."""
    z = qnet.act_block[0](action)
    emb = z / (1.0 + torch.exp(-z))
    x = torch.cat([_chain(qnet.in_block, state), emb], dim=1)
    return qnet.q_out_layer(_chain(qnet.q_block, x))[:, 0]


def gumbel(u):
    return -torch.log(-torch.log(u + GUMBEL_EPS) + GUMBEL_EPS)


class _Adam:
    """torch.optim.Adam's defaults: betas 0.9 / 0.999, eps 1e-8 added outside the bias-corrected root."""

    def __init__(self, params):
        self.params = params
        self.m = [torch.zeros_like(p) for p in params]
        self.s = [torch.zeros_like(p) for p in params]
        self.step = 0

    def apply(self, grads, lr):
        self.step += 1
        bc1, bc2 = 1.0 - 0.9 ** self.step, 1.0 - 0.999 ** self.step
        with torch.no_grad():
            for p, g, m, s in zip(self.params, grads, self.m, self.s):
                m.mul_(0.9).add_(g, alpha=0.1)
                s.mul_(0.999).add_(g * g, alpha=0.001)
                p.sub_((lr / bc1) * m / (s.sqrt() / math.sqrt(bc2) + 1e-8))


class Yardstick:
    def __init__(self, parameter, lr, discount, loss_align_coeff, max_grad_norm, squashed, ls_range=None, dtype=torch.float64):
        """`parameter`: a sac_not.Parameter (copied, never modified).  ls_range: the log-scale clamp (lo, hi) in the log domain, None: no clamp."""
        self.policy = copy.deepcopy(parameter.policy).to("cpu").to(dtype)
        self.qnet = copy.deepcopy(parameter.qnet).to("cpu").to(dtype)
        self.dtype = dtype
        self.normal = hasattr(self.policy.policy_dist_block, "loc_layers")
        self.lr, self.discount, self.align, self.max_norm, self.squashed = lr, discount, loss_align_coeff, max_grad_norm, squashed
        self.ls_lo, self.ls_hi = ls_range if ls_range is not None else (-math.inf, math.inf)
        self.p_params, self.q_params = list(self.policy.parameters()), list(self.qnet.parameters())
        self.adam_p, self.adam_q = _Adam(self.p_params), _Adam(self.q_params)

    # ---- the head: an action from the raw outputs and one noise plane ------------------------------------------------------------------------------------
    def _ls_margins(self, ls_raw, margins):
        if math.isfinite(self.ls_lo):
            margins.append(float((ls_raw - self.ls_lo).abs().min()))
            margins.append(float((ls_raw - self.ls_hi).abs().min()))

    def _normal_action(self, head, e, margins):
        loc, ls_raw = head
        self._ls_margins(ls_raw.detach(), margins)
        inside = ((ls_raw >= self.ls_lo) & (ls_raw <= self.ls_hi)).to(self.dtype)  # (torch.clamp passes the gradient on the closed interval)
        ls = ls_raw * inside + (ls_raw.detach().clamp(self.ls_lo, self.ls_hi) * (1.0 - inside))
        x = loc + torch.exp(ls) * e
        return torch.tanh(x) if self.squashed else x

    def forward(self, state, action=None):
        """Head outputs as srlx_notsac_forward writes them (logits, or locs and CLAMPED log-scales), and q(s, action) when an action is given."""
        with torch.no_grad():
            head = policy_forward(self.policy, state.to(self.dtype))
            out = (head[0], head[1].clamp(self.ls_lo, self.ls_hi)) if self.normal else head
            q = q_forward(self.qnet, state.to(self.dtype), action.to(self.dtype)) if action is not None else None
        return out, q

    def _clip_and_step(self, params, adam, margins, step_on=None):
        raw = [p.grad.detach().clone() for p in params]
        norm = math.sqrt(sum(float((g ** 2).sum()) for g in raw))
        margins.append(abs(norm / self.max_norm - 1.0))
        coef = min(1.0, self.max_norm / (norm + 1e-6))
        grads = [g * coef for g in raw]
        adam.apply(grads if step_on is None else [g.detach().to("cpu").to(self.dtype) for g in step_on], self.lr)
        return raw, grads, norm

    def update(self, state, n_state, action, reward, not_terminated, total_reward, noise, lr=None, step_on=None):
        """One training step on float64 CPU tensors: state / n_state [B][D]; action [B][A] one-hot or [B][K]; reward, not_terminated, total_reward [B];
        noise [2][B][K or A].  `step_on`: (Q gradients, policy gradients) after their clips that the two Adams step on INSTEAD of the yardstick's own."""
        dt = self.dtype
        if lr is not None:
            self.lr = lr
        state, n_state, action, noise = state.to(dt), n_state.to(dt), action.to(dt), noise.to(dt)
        B = state.shape[0]
        margins = []
        # ---- the target (:150-160)
        with torch.no_grad():
            n_head = policy_forward(self.policy, n_state)
            if self.normal:
                n_action = self._normal_action(n_head, noise[0], margins)
            else:
                noisy = n_head + gumbel(noise[0])
                top2 = torch.topk(noisy, 2, dim=1).values
                margins.append(float((top2[:, 0] - top2[:, 1]).min()))
                n_action = torch.nn.functional.one_hot(torch.argmax(noisy, dim=1), noisy.shape[1]).to(dt)
            n_q = q_forward(self.qnet, n_state, n_action)
        target = [float(reward[b]) + float(not_terminated[b]) * self.discount * float(n_q[b]) for b in range(B)]
        # ---- the Q step (:163-174): per-row losses and seeds; the target is the first argument and q takes the gradient
        q_t = q_forward(self.qnet, state, action)
        q = q_t.detach().tolist()
        s_hub = s_align = 0.0
        dq = []
        for b in range(B):
            d = target[b] - q[b]
            margins.append(abs(abs(d) - 1.0))
            if abs(d) < 1.0:
                s_hub += 0.5 * d * d
                g = -d
            else:
                s_hub += abs(d) - 0.5
                g = -math.copysign(1.0, d)
            e = float(total_reward[b]) - q[b]
            s_align += e * e
            dq.append((g + self.align * (-2.0 * e)) / B)
        for p in self.q_params:
            p.grad = None
        q_t.backward(torch.tensor(dq, dtype=dt))
        q_raw, q_grads, q_norm = self._clip_and_step(self.q_params, self.adam_q, margins, None if step_on is None else step_on[0])
        # ---- the policy step (:177-189), through the Q-network as it stands now
        head = policy_forward(self.policy, state)
        if self.normal:
            pi_action = self._normal_action(head, noise[1], margins)
        else:
            pi_action = torch.softmax(head + gumbel(noise[1]), dim=1)
        q_pi = q_forward(self.qnet, state, pi_action)
        for p in self.p_params:
            p.grad = None
        q_pi.backward(torch.full((B,), -1.0 / B, dtype=dt))
        loss_policy = -sum(q_pi.detach().tolist()) / B
        p_raw, p_grads, p_norm = self._clip_and_step(self.p_params, self.adam_p, margins, None if step_on is None else step_on[1])
        return dict(q=torch.tensor(q, dtype=dt), target_q=torch.tensor(target, dtype=dt), next_action=n_action, pi_action=pi_action.detach(),
                    loss_q=s_hub / B, loss_q_align=s_align / B, loss_policy=loss_policy, norm_q=q_norm, norm_policy=p_norm,
                    q_raw_grads=q_raw, q_grads=q_grads, p_raw_grads=p_raw, p_grads=p_grads, margin=min(margins),
                    q_params=[p.detach().clone() for p in self.q_params], p_params=[p.detach().clone() for p in self.p_params])
