"""Rank body of the multi-process front-door tests (`python -m torch.distributed.run ... tests/_sample_dist_worker.py <mode> <CLI flags>`).

Mode "cli": `vista_amd.sample.main` with the flags, as `-m vista_amd.sample` would run it, with every perform_save_locally call of this rank
written to $VISTA_TEST_LOG/rank<R>.log first (one line per call), so that the test sees who wrote what and how often.
Mode "rccl1" (world 1, VISTA_DIST_BACKEND=nccl): RCCL refuses two ranks on one GPU, so a one-GPU box puts the front door's sharded step through
RCCL itself with a frame-shard group of ONE rank in its `always_exchange` form (tests/_dist_worker.py has the reasoning): `sample.run(shard=)` on
the first sample of the dataset, latents saved to $VISTA_TEST_OUT, one JSON line with the collective counts."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cli(argv):
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    log = os.path.join(os.environ["VISTA_TEST_LOG"], f"rank{os.environ.get('RANK', '0')}.log")
    real = SU.perform_save_locally

    def logged(save_path, samples, mode, dataset_name, sample_index):
        with open(log, "a") as f:
            f.write(f"{os.path.relpath(save_path, os.environ['VISTA_TEST_LOG'])} {mode} {dataset_name} {sample_index}\n")
        return real(save_path, samples, mode, dataset_name, sample_index)
    SU.perform_save_locally = logged
    return sample.main(argv)


def rccl1(argv):
    import torch.distributed as dist
    from vista_amd import sample
    from vista_amd import sample_utils as SU
    from vista_amd.parallel import DistComm, FrameShard
    opt, _ = sample.parse_args().parse_known_args(argv)
    assert int(os.environ["WORLD_SIZE"]) == 1 and os.environ.get("VISTA_DIST_BACKEND", "nccl") == "nccl"
    dev = int(os.environ.get("VISTA_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
    try:
        shard = FrameShard(opt.n_frames, DistComm(dist.group.WORLD, name="frames[0..0]"), B=2)
        shard.always_exchange = True
        calls = {"all_to_all": 0, "all_reduce_sum": 0, "all_gather_list": 0}
        for name in calls:   # count what actually went through the process group
            def counted(*a, _f=getattr(shard.comm, name), _n=name, **k):
                calls[_n] += 1
                return _f(*a, **k)
            setattr(shard.comm, name, counted)
        shard.selfcheck(torch.device("cuda", dev))
        model = SU.init_model({"config": opt.config, "ckpt": opt.ckpt})
        sample.seed_everything(opt.seed)
        frame_list, _, _, action = SU.get_sample(0, opt.dataset, opt.n_frames, opt.action, data_root=opt.data_root, anno_file=opt.anno_file)
        _, samples_z, _ = sample.run(model, frame_list, action, height=opt.height, width=opt.width, n_frames=opt.n_frames, n_rounds=opt.n_rounds,
                                     n_conds=opt.n_conds, n_steps=opt.n_steps, cfg_scale=opt.cfg_scale, cond_aug=opt.cond_aug, shard=shard)
        torch.save(samples_z.cpu(), os.environ["VISTA_TEST_OUT"])
        print(json.dumps({"collective_calls": calls, "backend": shard.comm.backend}), flush=True)
    finally:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit({"cli": cli, "rccl1": rccl1}[sys.argv[1]](sys.argv[2:]))
