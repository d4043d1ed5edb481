"""Worker of tests/test_rel_stats_cpu.py: one of two gloo ranks.  Each counts its half of the fixture's training split,
all-reduces and writes the counts it ends with."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]


def main(rank, world, port, out_path):
    import rel_stats_inputs as RI
    from egtr_amd.statistics import RelationStatistics

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        targets = RI.train_targets()
        half = len(targets) // 2
        st = RelationStatistics(RI.C, RI.R)
        st.update(targets[:half] if rank == 0 else targets[half:])
        st.all_reduce()
        np.save(out_path, st.fg_matrix())
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
