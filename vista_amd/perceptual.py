"""CLIP-space scores of predicted frames, from the image tower every Vista checkpoint carries.

`conditioner.embedders.<i>.open_clip.model.visual.*` is the OpenCLIP ViT-H/14 image tower that conditions the UNet; the package runs it on its
own kernels (FrozenOpenCLIPImageEmbedder). Here the same tower embeds the 8-bit frames an evaluation scores -- the bytes of the saved pictures --
and three measures are formed in its embedding space:

  sim        per frame, the cosine of the predicted and the real frame's embeddings
  step       temporal consistency: the cosine of consecutive frames' embeddings (of the prediction, and of the real frames for comparison)
  mmd        a distribution distance between two sets of frames: the squared MMD with a Gaussian kernel (sigma 10) on normalised embeddings,
             times 1000, as in CMMD (Jayasumana et al., CVPR 2024)

What these numbers are not: the tower is ViT-H/14 at 224 px behind Vista's squashing resize (the whole frame resized to a square, no crop), so
the MMD is NOT comparable with published CMMD figures (ViT-L/14 at 336 px); the MMD of one scene (some 90 frames a side) is a small-sample
estimate, the run-level one over all frames is the one to read; and no real weights have been through it here (README "CLIP-space scores").

The frames go from bytes to the tower's patch operand in one kernel (ops.clip_preprocess_patches_u8), the tower runs in chunks of EMBED_CHUNK
frames in frame order, and the sums behind every score are fixed-order fp64 (ops.embed_row_stats, ops.embed_mmd_sums): the same bytes give the
same bits, online and from the saved pictures. The arithmetic from the sums to the scores is float64 on the host.
"""
from dataclasses import dataclass

import numpy as np

EMBED_CHUNK = 16            # frames per run of the tower; fixed, so that a stack is always cut the same way
SIGMA, SCALE = 10.0, 1000.0   # CMMD's kernel width and reporting scale


@dataclass
class PerceptualReport:
    sim: np.ndarray         # (n,) float64: cos(pred_i, real_i)
    step: np.ndarray        # (n,) float64: cos(pred_i, pred_{i-1}); entry 0 is NaN
    step_real: np.ndarray   # (n,) float64: cos(real_i, real_{i-1}); entry 0 is NaN
    mmd: dict = None        # mmd() of the scene's predicted against its real frames, where the caller formed it


# ---- the tower ------------------------------------------------------------------------------------------------------------------------------
def _is_tower(module):
    from .modules.encoders.modules import FrozenOpenCLIPImageEmbedder
    return isinstance(module, FrozenOpenCLIPImageEmbedder)


def find_tower(model):
    """The FrozenOpenCLIPImageEmbedder inside model.conditioner (the pipeline's own, weights and packs shared)."""
    for emb in model.conditioner.embedders:
        for cand in (emb, getattr(emb, "open_clip", None)):
            if cand is not None and _is_tower(cand):
                return cand
    raise ValueError("find_tower: the model's conditioner has no OpenCLIP image embedder; the CLIP-space scores need the checkpoint's image tower")


def _tower_entry(cfg):
    """-> (the checkpoint prefix of the image tower's tensors, the tower's own config) from the conditioner entry that holds it."""
    from .checkpoint import CONDITIONER_PREFIX
    embs = cfg["model"]["params"]["conditioner_config"]["params"]["emb_models"]
    for i, entry in enumerate(embs):
        inner = (entry.get("params") or {}).get("open_clip_embedding_config")
        if inner is not None and inner["target"].endswith("FrozenOpenCLIPImageEmbedder"):
            return f"{CONDITIONER_PREFIX}embedders.{i}.open_clip.", inner
    raise ValueError("load_tower: the config's conditioner lists no entry with an open_clip_embedding_config (the OpenCLIP image tower)")


def load_tower(config_path, ckpt):
    """The image tower alone, on the GPU: built from the conditioner entry of the config (None: the shipped one) and loaded, strictly, with
    the checkpoint's `conditioner.embedders.<i>.open_clip.*` tensors. No UNet and no first stage are built."""
    import torch
    from . import checkpoint, config
    from ._lib import VistaHipError
    from .pipeline import _plain
    from .util import instantiate_from_config
    if not torch.cuda.is_available():
        raise VistaHipError("load_tower: no GPU is visible; vista_amd runs on the MI355X only (no CPU / eager fallback)")
    prefix, entry = _tower_entry(_plain(config.load_config(config_path or config.CONFIG_PATH)))
    tower = instantiate_from_config(entry)
    own = {k[len(prefix):]: v for k, v in checkpoint.load_checkpoint(ckpt).items() if k.startswith(prefix)}
    if not own:
        raise KeyError(f"load_tower: {ckpt} holds no {prefix}* tensors")
    tower.load_state_dict(own, strict=True)
    return tower.cuda().eval()


def tower_info(tower):
    g = tower.geometry
    return {"embed": int(g["embed"]), "image": int(g["image"]), "patch": int(g["patch"]), "sigma": SIGMA, "scale": SCALE}


def embed_frames(tower, frames_u8):
    """frames_u8 (n, H, W, 3) uint8 on the GPU -> (n, E) fp32 on the GPU. Preprocessing from the bytes, then the tower, EMBED_CHUNK frames at
    a time in frame order: the launches are a function of the stack's shape alone."""
    import torch
    from . import ops

    @ops.bf16_storage   # (the conditioner stores bf16 in every process)
    def run(chunk):
        g = tower.geometry
        patches = ops.clip_preprocess_patches_u8(chunk, out_hw=g["image"], patch=g["patch"], antialias=tower.antialias)
        return tower.embed_patches(patches, chunk.shape[0])

    if frames_u8.dim() != 4 or frames_u8.shape[0] < 1:
        raise ValueError(f"embed_frames: expected an (n, H, W, 3) uint8 stack of at least one frame, got {tuple(frames_u8.shape)}")
    frames_u8 = frames_u8.contiguous()
    return torch.cat([run(frames_u8[i:i + EMBED_CHUNK]).float() for i in range(0, frames_u8.shape[0], EMBED_CHUNK)]).contiguous()


# ---- from the sums to the scores: float64, host -------------------------------------------------------------------------------------------------
def cosines(stats):
    """(n, 3) float64 rows of a.b, a.a, b.b -> (n,) cosines; NaN where a norm is zero or not finite."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cos = stats[:, 0] / np.sqrt(stats[:, 1] * stats[:, 2])
    cos[~(np.isfinite(cos) & np.isfinite(stats[:, 1]) & np.isfinite(stats[:, 2]))] = np.nan
    return cos


def _steps(e):
    from . import ops
    out = np.full(e.shape[0], np.nan, dtype=np.float64)
    if e.shape[0] > 1:
        out[1:] = cosines(ops.embed_row_stats(e[1:], e[:-1]).cpu().numpy())
    return out


def frame_scores(e_pred, e_real):
    """e_pred, e_real (n, E) fp32 embeddings on the GPU, paired by index -> PerceptualReport."""
    from . import ops
    if e_pred.shape != e_real.shape:
        raise ValueError(f"frame_scores: pred has {tuple(e_pred.shape)} embeddings, real {tuple(e_real.shape)}: the sets must pair up frame by frame")
    sim = cosines(ops.embed_row_stats(e_pred, e_real).cpu().numpy())
    return PerceptualReport(sim=sim, step=_steps(e_pred), step_real=_steps(e_real))


def mmd_from_sums(sums, m, n, scale=SCALE):
    """The three pair sums of ops.embed_mmd_sums (S_xx and S_yy over i < j, S_xy over all pairs, each of 1 - k) -> the squared MMD times
    `scale`: "biased" is the V-statistic (the diagonal, k = 1, included), "unbiased" the U-statistic, None where a side has one row."""
    sxx, syy, sxy = (float(v) for v in sums)
    m, n = int(m), int(n)
    biased = scale * (2.0 * sxy / (m * n) - 2.0 * sxx / (m * m) - 2.0 * syy / (n * n))
    unbiased = None
    if m > 1 and n > 1:
        unbiased = scale * (2.0 * sxy / (m * n) - 2.0 * sxx / (m * (m - 1)) - 2.0 * syy / (n * (n - 1)))
    return {"biased": biased, "unbiased": unbiased, "m": m, "n": n}


def mmd(e_x, e_y, sigma=SIGMA, scale=SCALE):
    """e_x (m, E), e_y (n, E) fp32 embeddings on the GPU -> {"biased", "unbiased", "m", "n"}: mmd_from_sums of ops.embed_mmd_sums. A row with
    a zero or non-finite norm makes the values NaN."""
    from . import ops
    sums = ops.embed_mmd_sums(e_x.contiguous(), e_y.contiguous(), sigma)
    return mmd_from_sums(sums.cpu().numpy(), e_x.shape[0], e_y.shape[0], scale)


def mmd_json(d):
    """mmd()'s dict for strict JSON: a value that is not finite is null."""
    fin = lambda v: None if v is None or not np.isfinite(v) else float(v)   # noqa: E731
    return {"biased": fin(d["biased"]), "unbiased": fin(d["unbiased"]), "m": int(d["m"]), "n": int(d["n"])}


# ---- one evaluation run ---------------------------------------------------------------------------------------------------------------------
class RunScores:
    """The CLIP-space side of an evaluation run: scores every scene and keeps the predicted frames' embeddings (4 KB a frame, on the GPU) for
    the run-level MMD. In a scene-per-rank run (frontdoor.RankedRun) every rank saves its scenes' embeddings with their walk positions
    (save_part: fp32 on the host) and rank 0 puts all of them back on its GPU in walk order (load_parts): the rows and their order are the
    single-process run's, and so are the bits of the run-level MMD."""

    def __init__(self, tower):
        self.tower, self.pred, self.real, self.positions = tower, [], [], []

    def scene(self, pred_u8, real_u8, n_conds, position=None):
        """Two (n, H, W, 3) uint8 stacks -> the scene's PerceptualReport, its MMD over the predicted (not the conditioning) frames.
        position: the scene's place in the walk, for a run whose scenes are spread over ranks."""
        e_pred, e_real = embed_frames(self.tower, pred_u8), embed_frames(self.tower, real_u8)
        report = frame_scores(e_pred, e_real)
        if e_pred.shape[0] > n_conds:
            report.mmd = mmd(e_pred[n_conds:], e_real[n_conds:])
            self.pred.append(e_pred[n_conds:])
            self.real.append(e_real[n_conds:])
            self.positions.append(position)
        return report

    def save_part(self, path):
        import torch
        if any(k is None for k in self.positions):
            raise ValueError("RunScores.save_part: a scene was scored without its walk position")
        torch.save({"positions": [int(k) for k in self.positions], "pred": [e.cpu() for e in self.pred], "real": [e.cpu() for e in self.real]}, path)

    def load_parts(self, paths):
        """The part files of ranks 0, 1, ... -> this object keeps every rank's embeddings, on the GPU, in walk order."""
        import os
        import torch
        held = {}
        for rank, path in enumerate(paths):
            if not os.path.isfile(path):
                raise FileNotFoundError(f"scene-per-rank merge: rank {rank} left no embeddings file {path}: the run is incomplete, nothing is merged")
            part = torch.load(path)
            for k, e_pred, e_real in zip(part["positions"], part["pred"], part["real"]):
                if k in held:
                    raise ValueError(f"scene-per-rank merge: rank {rank} holds the embeddings of position {k} in {path}, which are held already")
                held[k] = (e_pred, e_real)
        self.positions = sorted(held)
        self.pred, self.real = ([held[k][side].cuda() for k in self.positions] for side in (0, 1))

    def summary(self):
        """-> the `clip=` argument of evaluate.summarize."""
        import torch
        run = mmd(torch.cat(self.pred), torch.cat(self.real)) if self.pred else None
        return {"mmd": run, "tower": tower_info(self.tower)}
