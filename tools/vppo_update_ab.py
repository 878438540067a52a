"""A/B of srlx_vppo_update between two BUILDS of libsrlx on the seeded cases of tests/vppo_cases.py: every output of two updates per case (v, n_v, new_logpi, the
five scalars, every gradient tensor before and after the clip, every parameter and both Adam moments after each update), compared bit for bit.

    SRLX_LIB=/path/to/other/libsrlx.so python tools/vppo_update_ab.py --dump A.npz     # one process per build: the library is chosen at import
    python tools/vppo_update_ab.py --dump B.npz
    python tools/vppo_update_ab.py --compare A.npz B.npz --out profiles/vppo_normal_update_ab.json

Written for the factoring of normal_row's log-probability lines into srlxv::normal_logp: the proof that it changed no bit."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path):
    import torch

    import vppo_cases as C
    from simple_distributed_rl_amd.device.vppo import VppoUpdate

    out = {}
    for name in C.NAMES:
        p = C.make_parameter(name, "cuda")
        cfg, head = p.config, C.CASES[name][2]
        u = VppoUpdate(p, max_batch=C.CASES[name][0])
        for k, b in enumerate(C.make_batches(name)):
            f = lambda x: x.float().cuda()  # noqa: E731
            o = u.update(f(b["state"]), f(b["n_state"]), f(b["action"]) if head else b["action"].int().cuda(), f(b["old_logpi"]), f(b["reward"]),
                         f(b["not_terminated"]), f(b["total_reward"]), cfg.lr, cfg.discount, cfg.clip_range, cfg.entropy_weight, cfg.loss_align_coeff,
                         cfg.max_grad_norm, cfg.squashed_gaussian_policy)
            torch.cuda.synchronize()
            for q in ("v", "n_v", "new_logpi", "scalars"):
                out[f"{name}/{k}/{q}"] = o[q].cpu().numpy()
            for kind, tensors in (("raw", u.raw_grads), ("g", u.grads), ("p", u.params), ("m", u.exp_avg), ("v2", u.exp_avg_sq)):
                for j, t in enumerate(tensors):
                    out[f"{name}/{k}/{kind}.{j}"] = t.detach().cpu().numpy()
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays of {len(C.NAMES)} cases with {os.environ.get('SRLX_LIB') or 'the in-tree library'}")


def compare(a_path, b_path, out_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    cases = {}
    for key in sorted(a.files):
        name = key.split("/")[0]
        c = cases.setdefault(name, dict(arrays=0, elements=0, differing_elements=0, sha256=hashlib.sha256()))
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype == np.float32
        c["arrays"] += 1
        c["elements"] += x.size
        c["differing_elements"] += int((x.view(np.int32) != y.view(np.int32)).sum())
        c["sha256"].update(x.tobytes())
    for c in cases.values():
        c["sha256"] = c["sha256"].hexdigest()[:16]
    result = dict(what="srlx_vppo_update, two updates per seeded case of tests/vppo_cases.py: v, n_v, new_logpi, scalars, gradients before and after the clip, "
                       "parameters and Adam moments after each update, build A against build B, float32 bit patterns",
                  a=os.path.basename(a_path), b=os.path.basename(b_path), cases=cases, differing_elements=sum(c["differing_elements"] for c in cases.values()),
                  elements=sum(c["elements"] for c in cases.values()))
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: result[k] for k in ("elements", "differing_elements")}), "wrote", out_path)
    return result["differing_elements"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vppo_normal_update_ab.json"))
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
    if args.compare:
        sys.exit(1 if compare(args.compare[0], args.compare[1], args.out) else 0)


if __name__ == "__main__":
    main()
