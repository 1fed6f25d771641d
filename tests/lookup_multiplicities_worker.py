"""Worker of tests/test_gpu_lookup_multiplicities.py: one rank of a coset-sharded proof made WITHOUT a multiplicity column
(launched by torch.distributed.run; the ranks share one GPU, backend gloo).  Every rank counts the column on its own replicated
columns.  Writes this rank's proof to <out>/proof_<rank>.npy and its counted column to <out>/column_<rank>.npy."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_dir, name, fri, cap, sec = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    import torch.distributed as dist
    import era_boojum_amd as E
    import satisfiability_cases as K
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = rank % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    circuit = K.circuit(name)
    ctx = E.Context(dev)
    setup = E.ProverSetup(ctx, circuit, fri, cap, sec, comm=E.TorchComm(ctx))
    np.save(os.path.join(out_dir, "column_%d.npy" % rank), setup.count_multiplicities())
    proof, _ = setup.prove(count_multiplicities=True)
    assert setup.last_workspace["overflow_slabs"] == 0
    np.save(os.path.join(out_dir, "proof_%d.npy" % rank), proof)
    setup.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
