"""What the GPU tests of PPO's fused actor-critic (csrc/srlx_ppo_net.hip) share about their float64 yardstick, for both policy heads: tests/test_ppo_net_gpu.py,
tests/test_ppo_discrete_gpu.py, tests/test_ppo_envelope_gpu.py.  Not a test module."""
import copy

KINK_MARGIN = 1e-5


def kink_margin(torch, net, x):
    """The smallest |pre-activation| of every row of x [n][obs] over the four ReLU layers of `net` (an ActorCritic with the default blocks), computed in float64
    on a copy of it.  A pre-activation within float32 rounding of zero takes the other ReLU branch in float64 (measured: 1e-8 among 8192 x 256 pre-activations, which
    moved the value block's gradient by 5e-4 of its largest entry) -- a property of the yardstick's precision, not of the kernel: the gradient tests keep the rows
    whose margin is above KINK_MARGIN."""
    with torch.no_grad():
        n64 = copy.deepcopy(net).double()
        x64 = x.double()
        z1 = n64.hidden_block[0](x64)
        z2 = n64.hidden_block[2](torch.relu(z1))
        h64 = torch.relu(z2)
        return torch.stack([z.abs().min(dim=1).values for z in (z1, z2, n64.value_block[0](h64), n64.policy_block[0](h64))]).min(dim=0).values


def rows_off_the_kinks(torch, net, x):
    """Indices of the rows of x whose every pre-activation lies further than KINK_MARGIN from zero in float64."""
    return torch.nonzero(kink_margin(torch, net, x) > KINK_MARGIN).reshape(-1)
