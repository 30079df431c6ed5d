"""Dev probe: the f16 ensemble forward with and without the input image of h3_ximage_kernel (cmbpo_set_ens_f16_image_min_rows
1 / -1), alternating, HIP events around `iters` launches.    python tools/probe_h3_image.py [rows,rows,...] [reps] [iters] [out.json]
Rows travel through a row list (a permutation of the branch slots), as in a rollout."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib, synthetic
from cmbpo_amd.pens import PE

sizes = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 10000, 20000, 35000, 100000]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
out_path = sys.argv[4] if len(sys.argv) > 4 else None
task = "AntSafe-v2"
obs_dim, act_dim = synthetic.ENV_DIMS[task]
rng = np.random.default_rng(0)
E = 7
ws, bs = synthetic.ensemble_weights(rng, E, obs_dim + act_dim, 512, 2 * (obs_dim + 1), bias_scale=0.05)
m = PE(obs_dim + act_dim, obs_dim + 1, hidden_dims=(512, 512), num_networks=E, num_elites=5, loss="MSPE",
       use_scaler_in=True, use_scaler_out=True, device="cuda:0")
m.set_weights(ws, bs, synthetic.scaler(rng, obs_dim + act_dim), synthetic.scaler(rng, obs_dim + 1))
lib = _lib.lib()
dev = torch.device("cuda:0")
result = {}
for B in sizes:
    obs = torch.randn(B, obs_dim, device=dev) * 0.5
    act = torch.rand(B, act_dim, device=dev) * 2 - 1
    rows = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
    mean = torch.empty(E, B, obs_dim + 1, device=dev)
    var = torch.empty_like(mean)

    def forward():
        _lib.check(lib.cmbpo_ens_forward(m.mlp.handle, _lib.ptr(obs), obs_dim, _lib.ptr(act), act_dim, _lib.ptr(rows), None, B,
                                         B, _lib.ptr(mean), _lib.ptr(var), _lib.current_stream()), "cmbpo_ens_forward")

    times = {"on": [], "off": []}
    for rep in range(reps):
        for name, setting in (("off", -1), ("on", 1)):
            lib.cmbpo_set_ens_f16_image_min_rows(setting)
            for _ in range(3):
                forward()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                forward()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    lib.cmbpo_set_ens_f16_image_min_rows(0)
    on, off = np.array(times["on"]), np.array(times["off"])
    result[str(B)] = {"on_us": [round(v, 2) for v in on], "off_us": [round(v, 2) for v in off],
                      "median_on": round(float(np.median(on)), 2), "median_off": round(float(np.median(off)), 2),
                      "off_spread": round(float(off.max() - off.min()), 2)}
    print(f"rows {B}: off {np.median(off):.1f} us (spread {off.max() - off.min():.1f})  on {np.median(on):.1f} us  "
          f"ratio {np.median(on) / np.median(off):.4f}", flush=True)
if out_path:
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
