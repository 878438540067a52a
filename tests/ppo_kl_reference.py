"""PPO's adaptive-KL surrogate (surrogate_type "kl": srl/algorithms/ppo/ppo.py:138-146, :279-287; srl/rl/tf/functions.py:86-103) restated for the tests of
csrc/srlx_ppo_math.h's KL functions: the same numbers, as torch graphs whose precision is the precision of their inputs (the yardstick runs them in float64).
Not a test module."""
PROB_FLOOR = 1e-10  # functions.py:88-89
BETA_START = 0.5    # ppo.py:177


def kl_categorical(torch, old_probs, new_probs):
    """functions.py:86-92: sum_k q_k log(q_k / p_k) with q, p clipped to [1e-10, 1]; torch.clamp passes the gradient where 1e-10 <= p <= 1, bounds included, as
    tf.clip_by_value does.  One value per row."""
    q, p = torch.clamp(old_probs, PROB_FLOOR, 1.0), torch.clamp(new_probs, PROB_FLOOR, 1.0)
    return (q * torch.log(q / p)).sum(-1)


def kl_normal(torch, m1, ls1, m2, ls2):
    """functions.py:95-103 (tfp's Normal.kl_divergence in closed form), per action dimension; ls1 / ls2: the log-scales as clamped."""
    return (ls2 - ls1) + (torch.exp(2 * ls1) + (m1 - m2) ** 2) * 0.5 * torch.exp(-2 * ls2) - 0.5


def adapt_beta(beta, kl_mean, target):
    """ppo.py:279-287"""
    if kl_mean < target / 1.5:
        return beta / 2
    if kl_mean > target * 1.5 and beta < 10:
        return beta * 2
    return beta


def _value_and_entropy(torch, lp, v, vt, ov, vclip, vc, vw, ew):
    if vclip:
        v_c = torch.maximum(torch.minimum(v, ov + vc), ov - vc)
        value = torch.maximum((v - vt) ** 2, (v_c - vt) ** 2)
    else:
        value = (v - vt) ** 2
    return vw * value.mean(), ew * -(-(torch.exp(lp) * lp)).sum(-1).mean()


def torch_loss_categorical(torch, logits, actions, old_lp, old_probs, adv, v, vt, ov, base, vclip, vc, vw, ew, beta):
    """compute_train_loss under "kl" for a categorical head: (policy, value, entropy, kl_mean); policy + value + entropy is what the seeds differentiate."""
    logp = torch.log_softmax(logits, dim=-1)
    lp = logp.gather(1, actions.long().view(-1, 1))
    ad = (adv - v.detach() if base else adv).view(-1, 1)
    kl = kl_categorical(torch, old_probs, torch.exp(logp))
    pol = torch.exp(lp - old_lp.view(-1, 1)).view(-1) * ad.view(-1) - beta * kl
    value, ent = _value_and_entropy(torch, lp, v, vt, ov, vclip, vc, vw, ew)
    return -pol.mean(), value, ent, kl.mean()


def torch_loss_normal(torch, loc, ls_raw, ls_range, action, old_lp, old_loc, old_ls, adv, v, vt, ov, base, vclip, vc, vw, ew, beta):
    """The same for a Normal head: every tensor [B][A] but adv / v / vt / ov [B]; the new log-scale is clamped inside the graph (the clamp gates its gradient)."""
    import math

    ls = torch.clamp(ls_raw, ls_range[0], ls_range[1])
    lp = -0.5 * math.log(2 * math.pi) - ls - 0.5 * ((action - loc) / torch.exp(ls)) ** 2
    ad = (adv - v.detach() if base else adv)[:, None]
    kl = kl_normal(torch, old_loc, old_ls, loc, ls)
    pol = torch.exp(lp - old_lp) * ad - beta * kl
    value, ent = _value_and_entropy(torch, lp, v, vt, ov, vclip, vc, vw, ew)
    return -pol.mean(), value, ent, kl.mean()
