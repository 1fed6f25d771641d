"""Worker of tests/test_gpu_copy_constraints.py: one rank of a coset-sharded setup (launched by torch.distributed.run; the ranks
share one GPU, backend gloo).  Every rank checks the copy constraints of an honest and of a changed witness on its own replicated
columns and writes both reports to <out>/reports_<rank>.json."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_dir, col, row = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    import torch
    import torch.distributed as dist
    import era_boojum_amd as E
    import copy_constraint_cases as CC
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = rank % torch.cuda.device_count()
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    circuit, _ = CC.free_circuit()
    ctx = E.Context(dev)
    setup = E.ProverSetup(ctx, circuit, 8, 16, 30, comm=E.TorchComm(ctx))
    reports = []
    for variables in (circuit.variables, CC.changed(circuit.variables, col, row)):
        d_v = ctx.upload(variables)
        r = setup.check_copy_constraints(d_v)
        ctx.free(d_v)
        reports.append([r.kind, r.column, r.row, r.partner_column, r.partner_row, r.value, r.partner_value, r.variable, list(r.failures)])
    with open(os.path.join(out_dir, "reports_%d.json" % rank), "w") as f:
        json.dump(reports, f)
    setup.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
