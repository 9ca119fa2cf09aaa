"""The workload of profiles/r31_feature_transport_kernels.txt: 25 calls of pvo_feature_transport on tools/feature_transport_bench.py's
pyramid (the VKITTI levels, C = 256, fp16, with cur, the disparity as the key), the device idle before each, for a kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o ft -- python tools/feature_transport_workload.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import feature_transport_bench as fb  # noqa: E402
from pvo_amd import droid_backends as db  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("feature_transport_workload needs the GPU (there is no fallback)")
dev = torch.device("cuda:0")
flow, disp, ref, cur = fb.make_operands(dev)
scales = [(W / fb.WD, H / fb.HT) for H, W in fb.LEVELS]
outs = [torch.empty(1, H, W, 2 * fb.C, dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for H, W in fb.LEVELS]
srcs = [torch.empty(H, W, dtype=torch.int32, device=dev) for H, W in fb.LEVELS]
for _ in range(25):
    db.feature_transport(ref, cur, flow, scales=scales, depth=disp, order=-1, out=(outs, srcs))
    torch.cuda.synchronize()
print("done")
