"""one score (both directions) of the clouds scripts/cloud_eval_timing.py kept: the workload of the kernel trace
    rocprofv3 --kernel-trace --stats -- python scripts/cloud_eval_trace_workload.py clouds.npz"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from gipuma_amd import cloud_eval
z = np.load(sys.argv[1])
s = cloud_eval.score(z["cloud"], z["reference"], 20.0)
print(s["accuracy_device_ms"], s["completeness_device_ms"], s["accuracy_search"])
