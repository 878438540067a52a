"""oracle/_golden_record.py -- TEST INFRASTRUCTURE ONLY.  What the golden recipes (oracle/gen_golden*.py) share: where the reference is, where the fixtures go,
and the recorder of one hand-fed `Trainer.train()`.  Importing this module needs numpy alone; torch and the reference are imported when a recipe runs."""
import argparse
import os
import sys

import numpy as np

ORACLE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(ORACLE, "..", "tests", "golden")
if os.path.join(ORACLE, "..", "tests") not in sys.path:  # tests/*_recipe.py: the inputs that recipes and tests share
    sys.path.insert(0, os.path.join(ORACLE, "..", "tests"))


def reference_root():
    """The directory that holds the reference's `srl` package: $SRL_REFERENCE, or /root/reference."""
    ref = os.environ.get("SRL_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "srl", "__init__.py")):
        raise SystemExit(f"no reference at {ref!r} (no srl/__init__.py): set SRL_REFERENCE to a checkout of pocokhc/simple_distributed_rl")
    return ref


def use_reference():
    """Makes `import srl` find the reference (and nothing write bytecode into its tree)."""
    sys.dont_write_bytecode = True
    for p in (ORACLE, reference_root()):
        if p not in sys.path:
            sys.path.insert(0, p)


def start(doc, more_arguments=None):
    """What every runnable recipe does first.  `python oracle/gen_golden_X.py [OUT]` writes its fixtures into OUT (default tests/golden) and nowhere else; the
    reference is on sys.path; torch computes with the 8 threads the fixtures were recorded with, whatever the machine and OMP_NUM_THREADS say (a reduction split
    over another number of threads rounds differently, and tests/test_golden_recipes.py compares bytes)."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", nargs="?", default=GOLDEN, help="directory the .npz files are written to (default: tests/golden)")
    if more_arguments is not None:
        more_arguments(ap)
    args = ap.parse_args()
    use_reference()
    import torch

    torch.set_num_threads(8)
    os.makedirs(args.out, exist_ok=True)
    return args


def run(main, doc):
    """`if __name__ == "__main__": run(main, __doc__)`"""
    main(start(doc).out)


def register_envs():
    """The two environments of oracle/_golden_env.py, registered with the reference from outside its tree (srl/base/env/registration.py:116-136)."""
    from srl.base.env import registration

    registration.register("TinyImageEnvGolden", entry_point="_golden_env:TinyImageEnv", check_duplicate=False)
    registration.register("FlatGoldenEnv", entry_point="_golden_env:FlatGoldenEnv", check_duplicate=False)


_ABSENT = object()


def record_train_step(trainer, memory, batches, weights, nets, hook=None, q_net=None):
    """ONE `trainer.train()` of the reference on the hand-made `(batches, weights)`, with `train_count = 1` (not a target-sync step).

    nets    {name: torch module} whose gradients are wanted
    hook    (object, attribute, pick): that function is wrapped and `pick(what it returned)` is kept of every call (`calc_target_q`, `_update_q`)
    q_net   the module whose forward output is kept when it carries gradient (the online Q rows of s_0)
    Returns dict(priorities=what the trainer handed to memory.update, grads={(net, key): every p.grad as loss.backward() left it, caught at optimizer.step()},
    q=the Q rows or None, hooked=[...]).  Every patch, the process-wide one of torch.optim.Adam.step included, is undone on the way out."""
    import torch

    rec = dict(priorities=None, grads={}, q=None, hooked=[])
    owner = {id(p): (n, k) for n, m in nets.items() for k, p in m.named_parameters()}
    undo = []

    def patch(obj, name, wrap):
        undo.append((obj, name, vars(obj).get(name, _ABSENT)))  # absent: an instance attribute is about to shadow the class's method
        setattr(obj, name, wrap(getattr(obj, name)))

    def keep_hooked(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            rec["hooked"].append(np.asarray(hook[2](out)).copy())
            return out
        return wrapped

    def keep_q(fn):
        def wrapped(*a, **k):
            y = fn(*a, **k)
            if y.requires_grad:
                rec["q"] = y.detach().clone().numpy()
            return y
        return wrapped

    def keep_grads(fn):
        def wrapped(self, *a, **k):
            for g in self.param_groups:
                for p in g["params"]:
                    if p.grad is not None and id(p) in owner:
                        rec["grads"][owner[id(p)]] = p.grad.detach().clone().numpy()
            return fn(self, *a, **k)
        return wrapped

    adam_step = torch.optim.Adam.step
    try:
        n = len(batches)
        patch(memory, "sample", lambda fn: lambda *a, **k: (batches, weights.copy(), list(range(n))))
        patch(memory, "update", lambda fn: lambda update_args, priorities, step: rec.__setitem__("priorities", np.asarray(priorities).copy()))
        patch(memory, "is_warmup_needed", lambda fn: lambda: False)
        if hook is not None:
            patch(hook[0], hook[1], keep_hooked)
        if q_net is not None:
            patch(q_net, "forward", keep_q)
        torch.optim.Adam.step = keep_grads(adam_step)  # the class's method: every optimizer of the process, until the finally below
        trainer.train_count = 1
        trainer.train()
    finally:
        torch.optim.Adam.step = adam_step
        for obj, name, old in reversed(undo):
            if old is _ABSENT:
                delattr(obj, name)
            else:
                setattr(obj, name, old)
    return rec


def sampled_entries(save, prng, name, before, after, grad, step_sums):
    """One parameter tensor, as data: 2048 sampled positions (`pos.`), there the Adam step after - before (`upd.`) and the gradient (`grad.`), the gradient's
    float64 sum and largest magnitude (`gsum.`, `gmax.`); then either the step's float64 sums (`sum.`, `abs.`: train_step_rainbow84, train_step_dqn84) or
    the gradient's absolute sum (`gabs.`: train_step_agent57_light84)."""
    d = (after.astype(np.float64) - before.astype(np.float64)).reshape(-1)
    g = grad.astype(np.float64).reshape(-1)
    pos = np.sort(prng.choice(d.size, size=min(2048, d.size), replace=False))
    save["pos." + name] = pos.astype(np.int64)
    save["upd." + name] = d[pos].astype(np.float32)
    save["grad." + name] = g[pos].astype(np.float32)
    save["gsum." + name] = np.float64(g.sum())
    save["gmax." + name] = np.float64(np.abs(g).max())
    if step_sums:
        save["sum." + name] = np.float64(d.sum())
        save["abs." + name] = np.float64(np.abs(d).sum())
    else:
        save["gabs." + name] = np.float64(np.abs(g).sum())
