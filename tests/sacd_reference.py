"""The yardstick of discrete SAC's update: a float64 restatement of srl/algorithms/sac/sac_tf_discrete.py:158-243, written as a different program from
csrc/srlx_sacd.hip and from algorithms/sac.py's torch backend:
  * torch.float64 copies of the five modules on the CPU;
  * the reference's own (B * A)-row expansion, every one-hot row through the whole Q-network (the kernels may split the first layer);
  * torch.softmax and then log for the next state's log-probabilities (the kernels take z - logsumexp(z));
  * autograd (the kernels use closed forms);
  * torch.optim.Adam in float64;
  * the target sync as the list comprehension helper.model_soft_sync is.
It reads nothing from the reference tree."""
import copy

import torch

NETWORKS = ("policy", "q1_online", "q1_target", "q2_online", "q2_target")


def all_q(state, n_actions, q1_model, q2_model):
    """compute_discrete_all_q (:54-66)."""
    batch_size = state.shape[0]
    state_expand = torch.repeat_interleave(state, n_actions, dim=0)  # (B*A, state_dim)
    action_onehot = torch.nn.functional.one_hot(torch.arange(n_actions), n_actions).to(state.dtype).tile((batch_size, 1))  # (B*A, A)
    q1 = q1_model(state_expand, action_onehot)
    q2 = q2_model(state_expand, action_onehot)
    return torch.minimum(q1, q2).reshape(batch_size, n_actions)


class Yardstick:
    def __init__(self, parameter, lr_policy, lr_q, lr_alpha, discount, tau, auto_scale, target_entropy, dtype=torch.float64):
        """`parameter`: anything with the five modules and log_alpha (algorithms.sac.Parameter); copied, never touched.  `dtype=torch.float32` evaluates the same
        program in float32: how far float32 itself is from a bar (tests/test_sacd_gpu.py quotes it for the hard case)."""
        self.dtype = dtype
        for name in NETWORKS:
            setattr(self, name, copy.deepcopy(getattr(parameter, name)).to("cpu").to(dtype))
        self.log_alpha = parameter.log_alpha.detach().to("cpu").to(dtype).clone().requires_grad_(True)
        self.n_actions = self.policy.out_layer.out_features
        self.discount, self.tau, self.auto_scale, self.target_entropy = discount, tau, auto_scale, target_entropy
        for net in (self.policy, self.q1_online, self.q2_online):
            net.requires_grad_(True)
        self.q1_optimizer = torch.optim.Adam(self.q1_online.parameters(), lr=lr_q)
        self.q2_optimizer = torch.optim.Adam(self.q2_online.parameters(), lr=lr_q)
        self.policy_optimizer = torch.optim.Adam(self.policy.parameters(), lr=lr_policy)
        self.alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=lr_alpha)

    def update(self, state, onehot_action, n_state, reward, done, hard_sync):
        """CPU tensors (cast to the yardstick's dtype): state / n_state [B][D], one-hot actions [B][A], reward and done [B].  Returns every quantity of the update, the gradients as
        they were when the optimisers read them, and the probabilities it met (for the tests' distance-from-the-clip assertion)."""
        state, onehot_action, n_state, reward, done = (t.to(self.dtype) for t in (state, onehot_action, n_state, reward, done))
        reward, done = reward[:, None], done[:, None]
        alpha = torch.exp(self.log_alpha.detach())
        n_probs = torch.softmax(self.policy(n_state), dim=-1)
        n_log_probs = torch.log(n_probs)
        n_q_min = all_q(n_state, self.n_actions, self.q1_target, self.q2_target)
        n_q_min = torch.sum(n_probs * (n_q_min - alpha * n_log_probs), dim=-1, keepdim=True)
        target_q = (reward + (1 - done) * self.discount * n_q_min).detach()

        out = {"y": target_q[:, 0], "alpha": alpha.clone()}
        grads = {}
        for key, net, opt in (("q1", self.q1_online, self.q1_optimizer), ("q2", self.q2_online, self.q2_optimizer)):
            q = net(state, onehot_action)
            loss = torch.mean(torch.square(target_q - q))
            opt.zero_grad()
            loss.backward()
            grads[key + "_online"] = [p.grad.clone() for p in net.parameters()]
            opt.step()
            out[key], out[key + "_loss"] = q.detach()[:, 0], loss.detach()

        q_val = all_q(state, self.n_actions, self.q1_online, self.q2_online).detach()
        probs = torch.softmax(self.policy(state), dim=-1)
        log_probs = torch.log(torch.clip(probs, 10e-8, 1))
        entropy = -torch.sum(probs * log_probs, dim=-1, keepdim=True)
        policy_loss = torch.mean(torch.sum(probs * (alpha * log_probs - q_val), dim=-1))
        self.policy_optimizer.zero_grad()
        policy_loss.backward()
        grads["policy"] = [p.grad.clone() for p in self.policy.parameters()]
        self.policy_optimizer.step()
        out["entropy"], out["policy_loss"], out["probs"] = entropy.detach()[:, 0], policy_loss.detach(), probs.detach()

        out["alpha_loss"] = torch.zeros((), dtype=self.dtype)
        grads["log_alpha"] = torch.zeros((), dtype=self.dtype)
        if self.auto_scale:
            entropy_diff = self.target_entropy - entropy.detach()
            log_alpha_loss = -torch.mean(torch.exp(self.log_alpha) * entropy_diff)
            self.alpha_optimizer.zero_grad()
            log_alpha_loss.backward()
            grads["log_alpha"] = self.log_alpha.grad.clone()
            self.alpha_optimizer.step()
            out["alpha_loss"] = log_alpha_loss.detach()

        with torch.no_grad():
            for target, online in ((self.q1_target, self.q1_online), (self.q2_target, self.q2_online)):
                if hard_sync:
                    new = [w.clone() for w in online.parameters()]
                else:
                    new = [(1 - self.tau) * t + self.tau * w for t, w in zip(target.parameters(), online.parameters())]
                for t, w in zip(target.parameters(), new):
                    t.copy_(w)
        out["grads"] = grads
        return out
