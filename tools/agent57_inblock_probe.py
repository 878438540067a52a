"""Probe: Agent57's image block on libsrlx ("srlx": device/qnet.py:SeqImageTrunk) next to the torch module on MIOpen ("torch", the parent's path),
the measurement that decides QNetwork.in_block_backend's default.  Both arms keep the LSTM on libsrlx (QNetwork.lstm_backend's default).

    python tools/agent57_inblock_probe.py --out profiles/agent57_inblock_probe.json
    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/agent57_inblock_probe.py --trace-loop   # a run of its own, no counters

Three GPU steps, each a child process of its own under its own time limit (a step that fails or runs out of time ends the probe: nothing more is started on the
GPU).  Inside a step the two arms run in ONE process, interleaved three times, after one untimed call of each arm (allocation, MIOpen's solver search); every
timing ends in a device synchronise (tools/agent57_lstm_probe.py's scaffold):
  golden       one whole Trainer.train() at the shape of tests/golden/train_step_agent57.npz (B = 8, burn-in 2 + sequence 3 + 1, 8 x 8 frames)
  atari        one whole Trainer.train() at set_atari_config()'s shape (B = 64, 40 + 80 + 1 steps, 84 x 84 frames: 2 560 burn-in and 5 184 sequence rows)
  block_alone  the image block's forward + backward alone at 5 184 rows of 84 x 84 x 1 frames
The default rule (README): "srlx" iff atari.srlx_ms_mean <= 1.10 * atari.torch_ms_mean of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMITS = dict(golden=300, atari=600, block_alone=300)  # seconds per child
ARMS = ("srlx", "torch")


def _trainer(kind, backend):
    from agent57_lstm_probe import _trainer as lstm_probe_trainer

    trainer, nets, shape = lstm_probe_trainer(kind, "srlx")
    for net in nets:
        net.in_block_backend = backend
    return trainer, nets, shape


def _step_trainer(kind):
    from agent57_lstm_probe import _interleaved

    arms, shape, srlx_nets = {}, None, None
    for backend in ARMS:
        trainer, nets, shape = _trainer(kind, backend)
        srlx_nets = nets if backend == "srlx" else srlx_nets

        def run(trainer=trainer, nets=nets, backend=backend):
            trainer.train()
            assert all(n.in_block_path == backend for n in nets), [(n.in_block_path, n.why_not_srlx_in_block) for n in nets]
        arms[backend] = run
    res = dict(what="one whole Trainer.train() (host batch assembly included), ms", shape=shape, **_interleaved(arms))
    res["scratch_bytes_per_online_network"] = srlx_nets[0]._trunk.training_bytes  # (nets[0]: q_ext_online)
    return res


def _step_block_alone():
    import torch

    from agent57_lstm_probe import _interleaved
    from simple_distributed_rl_amd.device.qnet import SeqImageTrunk
    from simple_distributed_rl_amd.rl.torch_.networks import InputImageBlock

    rows, H = 64 * 81, 84
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = InputImageBlock((H, H, 1)).to(dev)
    frames = torch.rand((rows, H, H, 1), device=dev)
    g = torch.randn((rows, net.out_size), device=dev)
    trunk = SeqImageTrunk(net.image_block, (H, H), rows)

    def srlx():
        net.zero_grad()
        trunk.features(frames).backward(g)

    def torch_():
        net.zero_grad()
        net(frames).backward(g)
    res = dict(what="image block forward + backward alone (six parameter gradients), ms", shape=dict(rows=rows, frame=[H, H, 1]), **_interleaved(dict(srlx=srlx, torch=torch_)))
    res["scratch_bytes"] = trunk.training_bytes
    return res


def _trace_loop(steps):
    import torch

    trainer, nets, _ = _trainer("atari", "srlx")
    for _ in range(steps):
        trainer.train()
    torch.cuda.synchronize()
    assert all(n.in_block_path == "srlx" and n.lstm_path == "srlx" for n in nets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", default="golden,atari,block_alone")
    ap.add_argument("--child", default=None, help="(internal) run one GPU step in this process and print its JSON")
    ap.add_argument("--trace-loop", action="store_true", help="three Atari-shape trainer steps with both switches on 'srlx', for a profiler")
    a = ap.parse_args()
    if a.trace_loop:
        return _trace_loop(3)
    if a.child:
        res = _step_block_alone() if a.child == "block_alone" else _step_trainer(a.child)
        print("PROBE-JSON " + json.dumps(res))
        return
    from agent57_lstm_probe import run_steps

    run_steps(__file__, LIMITS, a.steps, a.out, "in_block_backend may default to 'srlx' iff the Atari-shape trainer step with it is at most 1.10 x the torch arm's in this run")


if __name__ == "__main__":
    main()
