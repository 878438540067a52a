"""A learner's forward passes (128 rows = the online pass, 96 rows = the target pass) with the first dense layer on three kernels:
  staging split   k_gemm_s16<APlain, .., H16>: float32 operands, split into float16 parts while staging
  planes, half-CU k_fc1_planes_h on borrowed operand planes, the launch padded to its 128-row tile (shaped for the actors' 1024 rows)
  planes, rows    k_fc1_planes_rows on the same planes (one row tile; what srlx_qnet_set_planes_small selects)
Per kernel: HIP-event time of a 128-row and a 96-row pass back to back (200 pairs) and the median bracket around the first dense layer's launch alone
(srlx_qnet_set_probe_fc1, 40 single passes each).  One JSON line; with a path as the first argument also written there."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from simple_distributed_rl_amd.device.qnet import EngineQNet, QNetInference

ROWS = (128, 96)
torch.manual_seed(0)
net = EngineQNet(6).cuda()
F = 84 * 84
g = torch.Generator(device="cuda").manual_seed(1)
ring = torch.randint(0, 256, (600 * F,), dtype=torch.uint8, device="cuda", generator=g)
offs = {rows: torch.randint(0, 600, (rows, 4), device="cuda", generator=g) * F for rows in ROWS}
pub = QNetInference(net, 128, 0)
actor = QNetInference(net, 512, 0)
actor.enable_fc1_planes(private_weights=True)
actor.enable_actor_sets()
pub.publish_to(actor, 1, with_fc1=True)
out, sums = {}, {}
for name, planes, half in (("staging_split", False, False), ("planes_half_cu", True, True), ("planes_rows", True, False)):
    hs = {}
    for rows in ROWS:
        h = QNetInference(net, rows, 0)
        if rows == 128:
            h.enable_training(32)  # (the online pass also writes what the backward pass reads)
        if planes:
            h.enable_fc1_planes(private_weights=False)
            h.set_planes_small(True, actor.set_planes_ptr(1), half_cu_kernel=half)
        hs[rows] = h
    for _ in range(10):
        qs = [hs[rows].forward_u8(ring.data_ptr(), offs[rows]) for rows in ROWS]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        qs = [hs[rows].forward_u8(ring.data_ptr(), offs[rows]) for rows in ROWS]
    b.record()
    torch.cuda.synchronize()
    res = {"pair_us": round(a.elapsed_time(b) / 200 * 1e3, 2)}
    for rows in ROWS:
        br = []
        for _ in range(40):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(), e1.record()  # (torch creates the HIP event at the first record)
            hs[rows].set_probe_fc1(e0, e1)
            hs[rows].forward_u8(ring.data_ptr(), offs[rows])
            torch.cuda.synchronize()
            br.append(e0.elapsed_time(e1) * 1e3)
        res[f"fc1_bracket_us_{rows}"] = round(statistics.median(br), 2)
    out[name] = res
    sums[name] = [float(q.double().sum()) for q in qs]
assert sums["staging_split"] == sums["planes_half_cu"] == sums["planes_rows"], sums  # (bit-identical kernels: equal checksums)
line = json.dumps({"tool": "learner_fc1_planes_time", "rows": list(ROWS), "kernels": out, "checksums_equal": True})
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
