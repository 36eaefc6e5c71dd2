import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
dev = torch.device("cuda", 0)
ev = lambda: torch.cuda.Event(enable_timing=True)
for i in range(3):
    print(json.dumps(bench.h264_picture_leg(torch, dev, ev)), flush=True)
