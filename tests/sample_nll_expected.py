"""Expected per-frame NLL of sampled frames, for tests/test_sample_nll_cpu.py and tests/test_gpu_sample_nll.py: the fp64 oracle's
teacher-forced pass (oracle.seqglow_oracle.seqglow_forward) over the seed's `start` frames followed by the generated ones. No new
fixture: every golden fixture already holds the reference's generated frames (infer/out) and the noise they were made from."""
import torch

from oracle import seqglow_oracle as oracle


def teacher_forced(hp, sd, data, frames, start):
    """-> (z (N, B, C), nll (N, B)) in fp64. data: inference()'s `data` ({modality: (B, >= seq_len, dim)}, p1_face: the seed);
    frames: (B, N, C) generated frames; seq_len = start + N."""
    seq_len = start + frames.shape[1]
    batch = {k: v[:, :seq_len].double() for k, v in data.items() if v.dim() == 3 and k != "p1_face"}
    batch["p1_face"] = torch.cat([data["p1_face"][:, :start].double(), frames.double().cpu()], 1)
    if hp["Conditioning"]["use_frame_nb"]:
        # inference() counts frames from one; forward() adds 2 * start to what the batch holds
        batch["frame_nb"] = torch.full((frames.shape[0], 1), 1.0 - 2 * start, dtype=torch.float64)
    z, _, nll = oracle.seqglow_forward(hp, {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}, batch)
    return z, nll


def fixture_expected(fx, frames=None):
    """The fixture's sampling case: (z, nll) of the reference's own generated frames (infer/out), or of `frames`."""
    data = {k: v.cpu() for k, v in fx.group("infer/data/").items()}
    return teacher_forced(fx.hp, fx.state_dict(), data, fx.get("infer/out") if frames is None else frames, fx.start)
