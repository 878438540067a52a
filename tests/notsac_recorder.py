"""Run by tests/test_notsac_pinned_cpu.py in a child interpreter that has the REFERENCE on its path ($SRL_REFERENCE): drives the reference's own
`srl.algorithms.sac_not` Trainer through two `train()` calls on hand-fed items and writes what it saw.  This project's code; it imports the reference and
contains none of its text.

    python tests/notsac_recorder.py DIR

DIR/cases.json lists the cases: name, env ("Grid" or "toy"), the Config's keyword arguments, the batch size, the torch seed of each step.  DIR/in_<name>.npz
holds the weights of both networks ("wp_<key>" / "wq_<key>" by state-dict key) and the items of both steps ("s<k>_<column>", the columns of
torch_model.py:238-251).  For every case DIR/out_<name>.npz receives: both state dicts before and after each step ("k<step>_before_p_<key>", ..._q_<key>,
"k<step>_after_..."), the batch as the trainer's *_np arrays hold it ("k<step>_<name>_np"), the reported losses ("k<step>_info_<key>"), every p.grad as each
of the two optimizer.step() calls found it ("k<step>_qgrad_<i>" then "k<step>_pgrad_<i>", in parameters() order), and the action argument of the Q-network's
three calls ("k<step>_qcall_<j>": the next action, the stored action, the policy's action), seen by a forward pre-hook: the reference stays untouched."""
import json
import os
import random
import sys

import numpy as np

COLUMNS = ("state", "n_state", "action", "reward", "not_done", "total_reward")
NP_ARRAYS = ("state_np", "n_state_np", "action_np", "reward_np", "not_terminated_np", "total_reward_np")


def _register_toy():
    """Observations of 3 floats, actions of 2 floats in [-1, 1]; the Trainer never steps it."""
    from srl.base.define import SpaceTypes
    from srl.base.env import registration
    from srl.base.env.base import EnvBase
    from srl.base.spaces.box import BoxSpace

    class NotSacPinToy(EnvBase):
        @property
        def action_space(self):
            return BoxSpace((2,), -1.0, 1.0, np.float32, SpaceTypes.CONTINUOUS)

        @property
        def observation_space(self):
            return BoxSpace((3,), -5.0, 5.0, np.float32, SpaceTypes.CONTINUOUS)

        @property
        def max_episode_steps(self):
            return 10

        @property
        def player_num(self):
            return 1

        def reset(self, **kw):
            return np.zeros(3, np.float32)

        def step(self, action):
            return np.zeros(3, np.float32), 0.0, True, False

        def backup(self, **kw):
            return None

        def restore(self, d, **kw):
            pass

    sys.modules[__name__].NotSacPinToy = NotSacPinToy
    registration.register("NotSacPinToy", entry_point=__name__ + ":NotSacPinToy", check_duplicate=False)
    return "NotSacPinToy"


def record(case, folder):
    import torch

    import srl
    from srl.algorithms import sac_not

    dat = np.load(os.path.join(folder, f"in_{case['name']}.npz"))
    B = case["batch_size"]
    cfg = sac_not.Config(batch_size=B, **case["config"])
    cfg.memory.warmup_size = B
    cfg.memory.capacity = B  # a ring: the second step's items replace the first's, the batch is the whole memory
    runner = srl.Runner("Grid" if case["env"] == "Grid" else _register_toy(), cfg)
    runner.set_device("CPU")
    trainer = runner.make_trainer()
    trainer.setup(runner.context)
    nets = {"p": trainer.parameter.policy, "q": trainer.parameter.qnet}
    out = {}
    for tag, net in nets.items():
        keys = list(net.state_dict())
        net.load_state_dict({k: torch.from_numpy(dat[f"w{tag}_" + k]) for k in keys})  # (by key, strict: this project's state dicts load into the reference's nets)
        out[f"keys_{tag}"] = np.array(keys)
    caught, qcalls = [], []
    adam_step = torch.optim.Adam.step

    def keep_grads(self, *a, **kw):
        caught.append([p.grad.detach().clone().numpy() for g in self.param_groups for p in g["params"]])
        return adam_step(self, *a, **kw)

    hook = nets["q"].register_forward_pre_hook(lambda module, args: qcalls.append(args[1].detach().clone().numpy()))
    torch.optim.Adam.step = keep_grads
    try:
        random.seed(5)
        for k in range(2):
            for i in range(B):
                item = [dat[f"s{k}_{c}"][i] for c in COLUMNS]
                item[3], item[4], item[5] = float(item[3]), int(item[4]), float(item[5])
                trainer.memory.add(item)
            for tag, net in nets.items():
                for key, t in net.state_dict().items():
                    out[f"k{k}_before_{tag}_{key}"] = t.detach().clone().numpy()
            del caught[:], qcalls[:]
            count = trainer.train_count
            torch.manual_seed(case["seeds"][k])
            trainer.train()
            assert trainer.train_count == count + 1 and len(caught) == 2 and len(qcalls) == 3, (trainer.train_count, len(caught), len(qcalls))
            for tag, net in nets.items():
                for key, t in net.state_dict().items():
                    out[f"k{k}_after_{tag}_{key}"] = t.detach().clone().numpy()
            for name in NP_ARRAYS:
                out[f"k{k}_{name}"] = getattr(trainer, name).copy()
            info = trainer.info.to_dict() if hasattr(trainer.info, "to_dict") else dict(trainer.info)
            for key, v in info.items():
                out[f"k{k}_info_{key}"] = np.float64(v)
            for tag, grads in zip(("q", "p"), caught):
                for i, g in enumerate(grads):
                    out[f"k{k}_{tag}grad_{i}"] = g
            for j, a in enumerate(qcalls):
                out[f"k{k}_qcall_{j}"] = a
    finally:
        torch.optim.Adam.step = adam_step
        hook.remove()
    np.savez(os.path.join(folder, f"out_{case['name']}.npz"), **out)


def main(folder):
    ref = os.environ["SRL_REFERENCE"]
    if ref not in sys.path:
        sys.path.insert(0, ref)
    import torch

    torch.set_num_threads(1)
    for case in json.load(open(os.path.join(folder, "cases.json"))):
        record(case, folder)
        print("recorded", case["name"])


if __name__ == "__main__":
    main(sys.argv[1])
