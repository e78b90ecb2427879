"""Self-critical sequence training (not in the reference): one step samples
n captions per image from the model, scores them on the host (CIDEr-D by
default), turns the scores into advantages against a baseline, and runs one
optimizer step on the sampled captions weighted by their advantages
(TrainEngine.step_weighted): the REINFORCE estimate of the expected reward's
gradient, loss = mean over all caption positions of -A * log p(token).

Cost per step: one sampled decode (SampleDecoder: encoder + max_seq_len - 1
positions on the K/V cache), the rewards on the host, one weighted training
step. The rewards need the sampled ids on the host, so every step has ONE
host synchronisation (the decode's read-back) that the cross-entropy step
does not have; that is inherent in a host-side reward. The loss stays on
the device.
"""
from __future__ import annotations

import numpy as np
import torch

BASELINES = ("mean", "greedy")


def advantages(rewards, baseline="mean", greedy=None):
    """rewards (B, n) -> (advantages (B, n), baselines (B, n)), float64.
    "mean": A_s = r_s - mean of the image's OTHER samples (n >= 2; a sample
    is not its own baseline, so the estimate stays unbiased). "greedy":
    A_s = r_s - greedy[i], the reward of the image's greedy caption."""
    r = np.asarray(rewards, dtype=np.float64)
    if r.ndim != 2:
        raise ValueError(f"rewards must be (images, samples), got {r.shape}")
    n = r.shape[1]
    if baseline == "mean":
        if n < 2:
            raise ValueError('baseline="mean" needs n_samples >= 2')
        base = (r.sum(axis=1, keepdims=True) - r) / (n - 1)
    elif baseline == "greedy":
        g = np.asarray(greedy, dtype=np.float64)
        if g.shape != (r.shape[0],):
            raise ValueError(f"greedy rewards must be ({r.shape[0]},), got {g.shape}")
        base = np.broadcast_to(g[:, None], r.shape).copy()
    else:
        raise ValueError(f"baseline must be one of {BASELINES}, got {baseline!r}")
    return r - base, base


def pack_tokens(samples, width, start_token, end_token, max_tokens):
    """Sampled captions as padded training rows (len(samples), width) int64:
    <start> ids [<end> if the sample ended] 0... A sample (ids without
    <start> / <end>) ended iff it is shorter than max_tokens, the number of
    positions the sampler ran; rows are cut at width."""
    out = np.zeros((len(samples), width), dtype=np.int64)
    for r, ids in enumerate(samples):
        row = [start_token] + [int(t) for t in ids]
        if len(ids) < max_tokens:
            row.append(end_token)
        row = row[:width]
        out[r, :len(row)] = row
    return out


class SelfCriticalTrainer:
    """Ties sampling, reward and update together for one model / engine.
    Decoders are cached per (batch, n_samples, temperature, top_k, top_p);
    their graphs read the parameters by address, so they follow the updates."""

    def __init__(self, transformer, engine, start_token, end_token, max_seq_len):
        if max_seq_len < 2:
            raise ValueError("self-critical training needs max_seq_len >= 2")
        self.transformer, self.engine = transformer, engine
        self.start_token, self.end_token, self.max_seq_len = start_token, end_token, max_seq_len
        # <start> + the sampled tokens fill the positional table exactly, and
        # the token rows get the width of the training captions
        self.steps = max_seq_len - 1
        self._decoders = {}

    def _decoder(self, b, n, temperature, top_k, top_p):
        from .decode import SampleDecoder
        key = (b, n, float(temperature), int(top_k), float(top_p))
        dec = self._decoders.get(key)
        if dec is None:
            dec = self._decoders[key] = SampleDecoder(
                self.transformer, b, n, self.steps, self.start_token, self.end_token,
                use_graph=self.engine.use_graph, temperature=temperature, top_k=top_k, top_p=top_p)
        return dec

    def sample(self, img, n_samples, temperature=1.0, top_k=0, top_p=1.0, seed=None):
        """Per image n_samples (ids, log-probability) pairs (inference mode)."""
        return self._decoder(img.shape[0], n_samples, temperature, top_k, top_p).decode(img, seed=seed)

    def greedy(self, img):
        """The arg-max caption of every image (ties to the lowest id): a
        top_k = 1 sampler, which equals the reference decode."""
        return [s[0][0] for s in self._decoder(img.shape[0], 1, 1.0, 1, 1.0).decode(img, seed=0)]

    def step(self, img, refs, n_samples=5, baseline="mean", reward=None, temperature=1.0, top_k=0, top_p=1.0,
             seed=None):
        b = img.shape[0]
        if n_samples < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        if baseline not in BASELINES:
            raise ValueError(f"baseline must be one of {BASELINES}, got {baseline!r}")
        if baseline == "mean" and n_samples < 2:
            raise ValueError('baseline="mean" needs n_samples >= 2')
        if reward is None or refs is not None:
            if refs is None or len(refs) != b:
                raise ValueError(f"{b} images need {b} reference lists, got "
                                 f"{'none' if refs is None else len(refs)}")
        if reward is None:
            from utils.cider_reward import CiderDReward
            reward = CiderDReward.from_corpus(list(refs))  # document frequencies of this batch
        drawn = self.sample(img, n_samples, temperature, top_k, top_p, seed)
        ids = [s[0] for per in drawn for s in per]
        logp = np.array([s[1] for per in drawn for s in per], dtype=np.float64)
        r = np.array([float(reward(i, ids[i * n_samples + s])) for i in range(b) for s in range(n_samples)],
                     dtype=np.float64).reshape(b, n_samples)
        g = None
        if baseline == "greedy":
            g = np.array([float(reward(i, c)) for i, c in enumerate(self.greedy(img))], dtype=np.float64)
        adv, base = advantages(r, baseline, g)
        tok = pack_tokens(ids, self.max_seq_len, self.start_token, self.end_token, self.steps)
        dev = img.device
        loss = self.engine.step_weighted(img, torch.from_numpy(tok).to(dev),
                                         torch.from_numpy(adv.reshape(-1).astype(np.float32)).to(dev))
        return {"loss": loss, "reward_mean": float(r.mean()), "baseline_mean": float(base.mean()),
                "sample_logp_mean": float(logp.mean()), "samples": drawn, "advantages": adv}
