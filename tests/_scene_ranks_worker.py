"""Rank body for tests/test_scene_ranks_cpu.py: the shared scene-per-rank code of vista_amd/frontdoor.py (scene_ranks, SceneRanks.join,
RankedRun) around a stub body over a fake dataset of seven scenes. No GPU, no model. Started once as a plain process and once under
`python -m torch.distributed.run` with VISTA_SCENE_RANKS=1; the two must leave the same records and the same summary.

    tests/_scene_ranks_worker.py SAVE_DIR N_SCENES [--random_walk]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATASET_LENGTH = 7
RECORDS_NAME, SUMMARY_NAME = "things.jsonl", "things_summary.json"


def get_scene(index, dataset, n_frames, action, data_root=None, anno_file=None):
    """Reads nothing and draws nothing, like SU.get_sample's lookup in the annotation."""
    index %= DATASET_LENGTH
    return [f"scene{index}/f0.jpg"], index, DATASET_LENGTH, {"index": index}


def body(frame_list, index):
    """A scene's record from draws of torch's and numpy's generators, which the walk seeds before every scene and never draws from."""
    import numpy as np
    import torch
    return {"index": index, "frames": frame_list, "torch": float(torch.rand(1)), "numpy": float(np.random.rand()), "timings": {}}


def main():
    from vista_amd import frontdoor
    save, n_scenes = sys.argv[1], int(sys.argv[2])
    opt = argparse.Namespace(seed=23, dataset="NUSCENES", n_frames=4, action="traj", data_root="root", anno_file="anno.json",
                             rand_gen="--random_walk" in sys.argv[3:])
    ranks = frontdoor.scene_ranks("evaluate", "scene-per-rank evaluation with a merge of the records is not built", n_scenes).join()

    def summarize(records):
        open(os.path.join(save, f"summarized_by_rank{ranks.rank}"), "w").close()
        return {"scenes": len(records), "mean_torch": frontdoor.mean([r["torch"] for r in records]),
                "mean_numpy": frontdoor.mean([r["numpy"] for r in records])}
    try:
        run = frontdoor.RankedRun(ranks, save, RECORDS_NAME, SUMMARY_NAME, summarize)
        for k, (frame_list, index, _length, _action) in run.scenes(opt, get_scene, n_scenes):
            run.add(k, body(frame_list, index))
            print(f"{ranks.prefix}thing {index} at {k}", flush=True)
        run.finish()
    finally:
        ranks.leave()


if __name__ == "__main__":
    main()
