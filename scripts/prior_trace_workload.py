import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gipuma_amd import prior, synth
scan = synth.build_scan("C", n_src=8, device="cuda")
dev = [torch.from_numpy(n).cuda() for n in scan.gt_norm4[1:]]
for S in (2, 4, 8):
    for _ in range(3):
        _, info = prior.prior_from_views(scan.P_matrices[0], dev[:S], scan.P_matrices[1:1 + S], 1.0, 300.0, 800.0, return_info=True)
    print(S, info)
