"""Child process of tests/test_gpu_depth_eval.py: DepthEval.merge / all_gather in an RCCL group of one.

    python tests/depth_eval_child.py <port>
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main():
    import torch.distributed as dist
    from camradepth_amd import synth
    from camradepth_amd.metrics import DepthEval
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", sys.argv[1]
    torch.cuda.set_device(0)
    batches = []
    for seed in (0, 1):
        gt = synth.make_batch(2, 64, 96, seed, with_seg=False)["gt_full"]
        rs = np.random.RandomState(50 + seed)
        pred = 1.0 - (1.0 - gt) * torch.from_numpy(1.0 + 0.3 * rs.uniform(-1, 1, size=tuple(gt.shape))).float()
        batches.append((pred.cuda(), gt.cuda()))
    single, a, b = DepthEval(), DepthEval(), DepthEval()
    for p, g in batches:
        single.update(p, g)
    a.update(*batches[0])
    b.update(*batches[1])
    merged = a.merge(b)

    def same(x, y):
        return bool(np.array_equal(x.sums(), y.sums()) and x.per_frame(50.0) == y.per_frame(50.0) and x.result() == y.result()
                    and x.result(cap=30.0) == y.result(cap=30.0) and x.by_range() == y.by_range())

    out = {"merged_equal": same(merged, single)}
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    gathered = DepthEval()
    for p, g in batches:
        gathered.update(p, g)
    gathered.all_gather()
    out["gathered_equal"] = same(gathered, single)
    out["pooled_equal"] = gathered.result(pooled=True) == single.result(pooled=True) and single.result(pooled=True) is not None
    out["frames"] = [single.frames(), merged.frames(), gathered.frames()]
    empty = DepthEval().all_gather()                       # a rank without frames takes part in the collective all the same
    out["frames"][1] = merged.frames() + empty.frames()
    dist.destroy_process_group()
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
