"""The yardstick of V-PPO's update: a float64 restatement of srl/algorithms/ppo_v/torch_model.py:111-178 and of the two distribution blocks
(srl/rl/torch_/distributions/categorical_dist_block.py:53-68, normal_dist_block.py:11-29,121-145), written as a different program from the plugin and the
kernels: the losses and their derivatives with respect to v and the head's outputs are explicit per-row formulas in Python floats; autograd carries those seeds
through the MLP only; the norm clip and Adam are explicit formulas too.  tests/test_vppo_pinned_cpu.py holds it to the reference's own code.

Every update also reports how far its rows are from the kinks of the arithmetic (`margin`, the smallest relative distance) and on which side of each kink
its rows fall (`regions`): the comparisons against float32 code are only meaningful away from the kinks, and tests/test_vppo_cpu.py requires that of every case."""
import copy
import math

import numpy as np
import torch

LOG_2PI_HALF = 0.5 * math.log(2.0 * math.pi)
PROB_FLOOR, SQUASH_FLOOR = 1e-7, 1e-10


def _chain(block, x):
    for layer in block.hidden_layers:
        x = layer(x)
    return x


def forward(net, state):
    """v [B] and the head's raw outputs [B][A] or [B][2][k] (locs, raw log-scales) of a float64 copy of ppo_v's network, layer by layer."""
    x = _chain(net.hidden_block, _chain(net.in_block, state))
    v = net.value_out_layer(_chain(net.value_block, x))[:, 0]
    h = _chain(net.policy_block, x)
    dist = net.policy_dist_block
    if hasattr(dist, "loc_layers"):
        return v, torch.stack([dist.loc_layers[0](h), dist.log_scale_layers[0](h)], dim=1)
    return v, dist.h_layers[0](h)


def _rel(x, kink):
    return abs(x / kink - 1.0)


class Yardstick:
    def __init__(self, parameter, lr, discount, clip_range, entropy_weight, loss_align_coeff, max_grad_norm, squashed, ls_range=None, dtype=torch.float64):
        """`parameter`: a ppo_v.Parameter (copied, never modified).  ls_range: the log-scale clamp (lo, hi) in the log domain, None: no clamp."""
        self.net = copy.deepcopy(parameter.net).to("cpu").to(dtype)
        self.dtype = dtype
        self.normal = hasattr(self.net.policy_dist_block, "loc_layers")
        self.lr, self.discount, self.clip, self.ew, self.align, self.max_norm = lr, discount, clip_range, entropy_weight, loss_align_coeff, max_grad_norm
        self.squashed = squashed
        self.ls_lo, self.ls_hi = ls_range if ls_range is not None else (-math.inf, math.inf)
        self.params = list(self.net.parameters())
        self.m = [torch.zeros_like(p) for p in self.params]
        self.s = [torch.zeros_like(p) for p in self.params]
        self.step = 0

    # ---- one row's log-probabilities and their derivatives with respect to the head's outputs ----------------------------------------------------------
    def _row_logpi(self, head, action, reg, margins):
        if not self.normal:
            z = [float(x) for x in head]
            m = max(z)
            e = [math.exp(x - m) for x in z]
            tot = sum(e)
            p = [x / tot for x in e]
            a = int(action)
            margins.append(_rel(p[a], PROB_FLOOR))
            if p[a] >= PROB_FLOOR:  # clamp(p, 1e-7, 1): the gradient passes on the closed interval
                reg["p_inside"] += 1
                return [math.log(p[a])], [[(1.0 if k == a else 0.0) - p[k] for k in range(len(z))]]
            reg["p_below"] += 1
            return [math.log(PROB_FLOOR)], [[0.0] * len(z)]
        k = head.shape[1]
        corr = 0.0
        if self.squashed:
            for i in range(k):
                x = 1.0 - math.tanh(float(action[i])) ** 2
                margins.append(_rel(x, SQUASH_FLOOR) if x > 0 else 1.0)
                reg["squash_clamped" if x < SQUASH_FLOOR else "squash_inside"] += 1
                corr += math.log(min(max(x, SQUASH_FLOOR), 1.0))
        lps, ds = [], []
        for j in range(k):
            loc, lsr = float(head[0][j]), float(head[1][j])
            ls = min(max(lsr, self.ls_lo), self.ls_hi)
            inside = self.ls_lo <= lsr <= self.ls_hi
            if math.isfinite(self.ls_lo):
                margins.extend([_rel(lsr, self.ls_lo), _rel(lsr, self.ls_hi)])
                reg["ls_below" if lsr < self.ls_lo else ("ls_above" if lsr > self.ls_hi else "ls_inside")] += 1
            sd = math.exp(ls)
            u = (float(action[j]) - loc) / sd
            lps.append(-LOG_2PI_HALF - ls - 0.5 * u * u - corr)
            ds.append((u / sd, (u * u - 1.0) if inside else 0.0))  # d lp / d loc, d lp / d raw log-scale
        return lps, ds

    def update(self, state, n_state, action, old_logpi, reward, not_terminated, total_reward, step_on=None):
        """One training step on float64 CPU tensors: state / n_state [B][D]; action [B] indices or [B][k]; old_logpi [B][K]; reward, not_terminated,
        total_reward [B].  Returns the outputs, the four losses, the gradients before and after the clip, the norm, `margin` and `regions`.  `step_on`: clipped
        gradients that Adam steps on INSTEAD of the yardstick's own (a float32 backend's: its Adam is then checked apart from its sums)."""
        dt = self.dtype
        v_t, head_t = forward(self.net, state.to(dt))
        with torch.no_grad():
            nv_t, _ = forward(self.net, n_state.to(dt))
        v, nv, head = v_t.detach().numpy(), nv_t.numpy(), head_t.detach().numpy()
        B = state.shape[0]
        K = head.shape[2] if self.normal else 1
        N = B * K
        lo, hi = 1.0 - self.clip, 1.0 + self.clip
        reg = {k: 0 for k in ("p_inside", "p_below", "squash_clamped", "squash_inside", "ls_below", "ls_inside", "ls_above", "huber_quadratic", "huber_linear",
                              "ratio_below_adv+", "ratio_below_adv-", "ratio_inside_adv+", "ratio_inside_adv-", "ratio_above_adv+", "ratio_above_adv-")}
        margins = []
        s_hub = s_align = s_pol = s_ent = 0.0
        dv, dhead, new_logpi = np.zeros(B), np.zeros(head.shape), np.zeros((B, K))
        for b in range(B):
            lps, dlps = self._row_logpi(head[b], action[b], reg, margins)
            q = float(reward[b]) + float(not_terminated[b]) * self.discount * float(nv[b])
            adv = q - float(v[b])
            tr = float(total_reward[b])
            for j in range(K):
                lp = lps[j]
                new_logpi[b, j] = lp
                ratio = math.exp(lp - float(old_logpi[b][j]))
                # value losses: v is the target argument of both, and takes the gradient
                d = ratio * q - float(v[b])
                margins.append(_rel(abs(d), 1.0))
                if abs(d) < 1.0:
                    s_hub += 0.5 * d * d
                    dv[b] += -d / N
                    reg["huber_quadratic"] += 1
                else:
                    s_hub += abs(d) - 0.5
                    dv[b] += -math.copysign(1.0, d) / N
                    reg["huber_linear"] += 1
                e = ratio * tr - float(v[b])
                s_align += e * e
                dv[b] += self.align * (-2.0 * e) / N
                # the clipped surrogate: inside the interval both products are equal and the whole gradient passes
                margins.extend([_rel(ratio, lo), _rel(ratio, hi)])
                rc = min(max(ratio, lo), hi)
                lu, lc = ratio * adv, rc * adv
                s_pol += min(lu, lc)
                side = "inside" if lo <= ratio <= hi else ("below" if ratio < lo else "above")
                reg[f"ratio_{side}_adv{'+' if adv > 0 else '-'}"] += 1
                if side != "inside":
                    margins.append(abs(adv) / 1e-3 if abs(adv) < 1e-3 else 1.0)  # (a tie outside the interval is adv = 0)
                g_ratio = adv if (side == "inside" or lu < lc) else 0.0
                g_lp = -g_ratio * ratio / N
                if self.ew > 0:
                    s_ent += math.exp(lp) * lp
                    g_lp += self.ew * (math.exp(lp) * lp + math.exp(lp)) / B
                if self.normal:
                    dhead[b, 0, j] += g_lp * dlps[j][0]
                    dhead[b, 1, j] += g_lp * dlps[j][1]
                else:
                    dhead[b] += g_lp * np.asarray(dlps[j])
        out = dict(v=torch.tensor(v), n_v=torch.tensor(nv), new_logpi=torch.tensor(new_logpi), loss_value=s_hub / N, loss_v_align=s_align / N,
                   loss_policy=-s_pol / N, loss_e=(s_ent / B if self.ew > 0 else 0.0), head=torch.tensor(head))
        for p in self.params:
            p.grad = None
        torch.autograd.backward([v_t, head_t], [torch.tensor(dv, dtype=dt), torch.tensor(dhead, dtype=dt)])
        raw = [p.grad.detach().clone() for p in self.params]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in raw))
        margins.append(_rel(norm, self.max_norm))
        reg_norm = "norm_above" if norm > self.max_norm else "norm_below"
        coef = min(1.0, self.max_norm / (norm + 1e-6))
        grads = [g * coef for g in raw]
        stepped = grads if step_on is None else [g.detach().to("cpu").to(dt) for g in step_on]
        # Adam (torch.optim.Adam's defaults: betas 0.9 / 0.999, eps 1e-8 added outside the bias-corrected root)
        self.step += 1
        bc1, bc2 = 1.0 - 0.9 ** self.step, 1.0 - 0.999 ** self.step
        with torch.no_grad():
            for p, g, m, s in zip(self.params, stepped, self.m, self.s):
                m.mul_(0.9).add_(g, alpha=0.1)
                s.mul_(0.999).add_(g * g, alpha=0.001)
                p.sub_((self.lr / bc1) * m / (s.sqrt() / math.sqrt(bc2) + 1e-8))
        out.update(raw_grads=raw, grads=grads, norm=norm, margin=min(margins), regions=dict(reg, **{reg_norm: 1}),
                   params=[p.detach().clone() for p in self.params])
        return out
