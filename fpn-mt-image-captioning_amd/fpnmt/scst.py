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

With a fpnmt.cider_device.DeviceCiderD as the reward the scoring runs on the
device instead (fpnmt_ciderd_reward on the sampler's own state, then
fpnmt_scst_pack for the advantages and the token rows): such a step reads
nothing back and, once its graphs exist, is graph replays and launches only.
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
        self._dev_state = {}

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

    # ------------------------------------------------- device-side reward
    def _device_state(self, b, n, dev):
        """The static buffers of the device-reward path for (b, n): rewards,
        greedy rewards, advantages, token rows, the three means, the image
        index and its pinned staging ring."""
        key = (b, n, str(dev))
        st = self._dev_state.get(key)
        if st is None:
            st = self._dev_state[key] = {
                "reward": torch.zeros(b * n, dtype=torch.float64, device=dev),
                "greedy": torch.zeros(b, dtype=torch.float64, device=dev),
                "adv": torch.zeros(b * n, dtype=torch.float32, device=dev),
                "tok": torch.zeros((b * n, self.max_seq_len), dtype=torch.int64, device=dev),
                "scalars": torch.zeros(3, dtype=torch.float64, device=dev),
                "index": torch.arange(b, dtype=torch.int32, device=dev), "index_is": None,
                "stage": [(torch.empty(b, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(4)],
                "stage_at": 0,
            }
        return st

    def _upload_index(self, st, rows):
        """rows: the images' table rows as a list (None: 0 .. b - 1). The
        only host-to-device traffic of a device-reward step: one asynchronous
        copy from a pinned staging buffer, skipped when the index is the one
        already on the device."""
        want = None if rows is None else tuple(rows)
        if st["index_is"] == want:  # the buffer starts as 0 .. b - 1
            return
        buf, ev = st["stage"][st["stage_at"]]
        st["stage_at"] = (st["stage_at"] + 1) % len(st["stage"])
        if not ev.query():  # this buffer's copy of four uploads ago: long done
            ev.synchronize()
        buf.numpy()[:] = np.arange(buf.numel()) if rows is None else np.asarray(rows)
        st["index"].copy_(buf, non_blocking=True)
        ev.record()
        st["index_is"] = want

    def _step_device(self, img, table, image_keys, n, baseline, temperature, top_k, top_p, seed):
        from ._lib import call, ptr, stream_ptr, SCST_MEAN, SCST_GREEDY
        from .cider_device import MAX_TOKEN
        b, dev = img.shape[0], img.device
        if table.device != dev:
            raise ValueError(f"the DeviceCiderD tables are on {table.device}, the images on {dev}")
        vocab = self.transformer.final_layer.kernel.shape[1]
        if vocab - 1 > MAX_TOKEN:
            raise ValueError(f"the packed n-gram keys hold token ids up to {MAX_TOKEN}, the vocabulary has {vocab}")
        if self.steps > table.max_len:
            raise ValueError(f"captions of up to max_seq_len - 1 = {self.steps} tokens exceed the tables' max_len "
                             f"{table.max_len}; build DeviceCiderD with max_len >= {self.steps}")
        if image_keys is None:
            if b > table.n_images:
                raise ValueError(f"{b} images index the first {b} table rows, the tables hold {table.n_images}; "
                                 "pass image_keys")
            rows = None
        else:
            if len(image_keys) != b:
                raise ValueError(f"{b} images need {b} image keys, got {len(image_keys)}")
            rows = table.rows_of(image_keys)  # an unknown key raises here, before any upload
        st = self._device_state(b, n, dev)
        self._upload_index(st, rows)
        if baseline == "greedy":
            hist, slen, fin, _ = self._decoder(b, 1, 1.0, 1, 1.0).decode_device(img, seed=0)
            table.reward(hist, slen, fin, st["index"], 1, st["greedy"])
        hist, slen, fin, score = self._decoder(b, n, temperature, top_k, top_p).decode_device(img, seed=seed)
        table.reward(hist, slen, fin, st["index"], n, st["reward"])
        call("fpnmt_scst_pack", b, n, SCST_GREEDY if baseline == "greedy" else SCST_MEAN, ptr(st["reward"]),
             ptr(st["greedy"]) if baseline == "greedy" else None, ptr(hist), hist.stride(0), ptr(slen), ptr(fin),
             ptr(score), self.start_token, self.end_token, self.steps, ptr(st["tok"]), self.max_seq_len,
             ptr(st["adv"]), ptr(st["scalars"]), stream_ptr())
        loss = self.engine.step_weighted(img, st["tok"], st["adv"])
        sc = st["scalars"].clone()
        return {"loss": loss, "rewards": st["reward"].clone().view(b, n), "advantages": st["adv"].clone().view(b, n),
                "reward_mean": sc[0], "baseline_mean": sc[1], "sample_logp_mean": sc[2],
                "hist": hist, "slen": slen, "fin": fin}

    def step(self, img, refs, n_samples=5, baseline="mean", reward=None, temperature=1.0, top_k=0, top_p=1.0,
             seed=None, image_keys=None):
        """One self-critical step. reward None / a callable: the host path
        (read-back, host scores, numpy advantages). reward a
        fpnmt.cider_device.DeviceCiderD: the device path — decode_device,
        fpnmt_ciderd_reward, fpnmt_scst_pack, step_weighted, with no read-back
        and no host synchronisation once the graphs exist (from the third
        call at a shape on); image_keys names the images' table rows (None:
        rows 0 .. B - 1) and refs is not needed. It returns device tensors:
        "loss", "rewards" (B, n) f64, "advantages" (B, n) fp32, the 0-dim
        "reward_mean" / "baseline_mean" / "sample_logp_mean", and the
        sampler's "hist" / "slen" / "fin" (valid until the next decode;
        fpnmt.decode.sampled_ids gives the id lists) — no "samples" list,
        which would be the read-back this path removes. reward "device":
        a DeviceCiderD built from this batch's refs every step (the document
        frequencies of reward None; host work for the tables, still no
        read-back) — a convenience; one corpus-level instance is the
        intended use."""
        b = img.shape[0]
        if n_samples < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        if baseline not in BASELINES:
            raise ValueError(f"baseline must be one of {BASELINES}, got {baseline!r}")
        if baseline == "mean" and n_samples < 2:
            raise ValueError('baseline="mean" needs n_samples >= 2')
        from .cider_device import DeviceCiderD
        if isinstance(reward, str):
            if reward != "device":
                raise ValueError(f'reward must be None, a callable, a DeviceCiderD or "device", got {reward!r}')
            if refs is None or len(refs) != b:
                raise ValueError(f"{b} images need {b} reference lists, got "
                                 f"{'none' if refs is None else len(refs)}")
            if image_keys is not None:
                raise ValueError('reward="device" scores image i against refs[i]; image_keys needs a DeviceCiderD')
            reward = DeviceCiderD.from_corpus(list(refs), img.device, max_len=max(self.steps, 1))
        if isinstance(reward, DeviceCiderD):
            return self._step_device(img, reward, image_keys, n_samples, baseline, temperature, top_k, top_p, seed)
        if image_keys is not None:
            raise ValueError("image_keys goes with a DeviceCiderD reward")
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
