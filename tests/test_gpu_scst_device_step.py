"""The self-critical step with the reward on the device
(Pipeline.train_step_scst(reward=<DeviceCiderD>)): against the host path on
an identically seeded model — the same samples, rewards within the kernel's
bound (tests/test_gpu_cider_reward.py), and, given the same advantages, the
same loss and parameters bit for bit (the step is bitwise deterministic,
DESIGN.md §6) —, its replay path without any host synchronisation, its
alternation with the plain and the host-reward step on one engine, and the
interface's errors. Shape: the existing step test's (1 layer, V = 300,
128^2, B = 2, n = 3, fp32)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
SC = dict(n_layers=1, vocab=300, image=128, T=10, B=2, n=3, end_bias=3.0)
STATE = ("flat", "m", "v", "vhat", "step")
LOW, HIGH = 4, 24  # the tokens the model is biased towards, and the references' vocabulary


def _corpus():
    """Six images, 2-4 references of 4-9 tokens over the favoured tokens."""
    rng = np.random.default_rng(5)
    return {f"img{i}": [rng.integers(LOW, HIGH, size=int(rng.integers(4, 10))).tolist()
                        for _ in range(int(rng.integers(2, 5)))] for i in range(6)}


def _images(b, image, seed):
    return (torch.rand(b, image, image, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _pipe(seed, lr, use_graph):
    """A small fp32 pipeline whose samples fall mostly on tokens LOW .. HIGH - 1
    (random weights would spread them over the vocabulary and nearly every
    reward would be 0)."""
    import fpnmt
    from fpnmt.layers import invalidate_weights
    from fpnmt.train import TrainEngine
    from test_gpu_beam_search import _pipeline
    fpnmt.set_precision("fp32")
    c = SC
    pl = _pipeline(c["n_layers"], c["vocab"], c["image"], seed, c["T"], c["end_bias"])
    with torch.no_grad():
        pl.transformer.final_layer.bias[LOW:HIGH] += 4.0
        pl.transformer.final_layer.bias[pl.end_token] += 5.0  # against twenty favoured tokens: <end> about 1 in 5
    invalidate_weights()
    pl.engine = pl.optimizer = TrainEngine(pl.transformer, lr, use_graph=use_graph)
    return pl


def _bound(cand_len, ref_lens, host):
    L = max([cand_len] + list(ref_lens))
    return 4.0 * (L + len(ref_lens) / 2.0 + 7.0) * U * host


@pytest.fixture(scope="module")
def tables():
    from fpnmt.cider_device import DeviceCiderD
    corpus = _corpus()
    return DeviceCiderD.from_corpus(corpus, DEV, max_len=16), corpus


@pytest.mark.parametrize("baseline", ["mean", "greedy"])
def test_device_reward_step_equals_the_host_path(tables, baseline):
    from fpnmt.decode import sampled_ids
    from fpnmt.scst import SelfCriticalTrainer, pack_tokens
    dev, corpus = tables
    c = SC
    keys = ["img4", "img1"]
    img = _images(c["B"], c["image"], 9)
    A, B = _pipe(31, 1e-4, False), _pipe(31, 1e-4, False)
    assert torch.equal(A.engine.arena.flat, B.engine.arena.flat)
    # B first: its sampler reads the parameters A's step is about to change in A only
    trB = SelfCriticalTrainer(B.transformer, B.engine, B.start_token, B.end_token, B.max_seq_len)
    drawn = trB.sample(img, c["n"], seed=7)
    ids = [s[0] for per in drawn for s in per]
    out = A.train_step_scst(img, None, n_samples=c["n"], baseline=baseline, reward=dev, image_keys=keys, seed=7)
    assert "samples" not in out
    assert sampled_ids(out["hist"], out["slen"], out["fin"]) == ids
    assert len({len(x) for x in ids}) > 1
    got = out["rewards"]
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (c["B"], c["n"])
    want = dev.host.score(keys, [[s[0] for s in per] for per in drawn]).reshape(c["B"], c["n"])
    r = got.cpu().numpy()
    for i, k in enumerate(keys):
        for s in range(c["n"]):
            if want[i, s] == 0.0:
                assert r[i, s] == 0.0
            else:
                assert abs(r[i, s] - want[i, s]) <= _bound(len(ids[i * c["n"] + s]), [len(x) for x in corpus[k]],
                                                          want[i, s])
    assert (want > 0).sum() >= 2, want
    adv = out["advantages"]
    assert adv.is_cuda and adv.dtype == torch.float32 and tuple(adv.shape) == (c["B"], c["n"])
    assert float(adv.abs().max()) > 0
    for name in ("reward_mean", "baseline_mean", "sample_logp_mean"):
        assert out[name].is_cuda and out[name].dim() == 0
    assert abs(float(out["reward_mean"]) - want.mean()) <= 1e-12 * max(1.0, want.mean())
    logp = np.array([s[1] for per in drawn for s in per], dtype=np.float64)
    assert abs(float(out["sample_logp_mean"]) - logp.mean()) <= 1e-12 * abs(logp.mean())
    # the same token rows and A's advantages through B's engine: the same step, bit for bit
    tok = torch.from_numpy(pack_tokens(ids, c["T"], B.start_token, B.end_token, c["T"] - 1)).to(DEV)
    loss_b = B.engine.step_weighted(img, tok, adv.reshape(-1).clone())
    torch.cuda.synchronize()
    assert torch.equal(out["loss"], loss_b), (float(out["loss"]), float(loss_b))
    for nme in STATE:
        assert torch.equal(getattr(A.engine.arena, nme), getattr(B.engine.arena, nme)), nme
    assert int(A.engine.arena.step) == 1


def test_replayed_device_reward_steps_never_wait_for_the_device(tables, monkeypatch):
    """The third and fourth call at a shape are graph replays and launches:
    torch's sync debug mode must not raise, and no tensor is read back
    (tolist / item / cpu counted, for a torch build that does not honour the
    mode for some call). lr 0: the same seed repeats its draws."""
    dev, _ = tables
    c = SC
    img = _images(c["B"], c["image"], 10)
    pl = _pipe(33, 0.0, True)
    kw = dict(n_samples=c["n"], reward=dev, baseline="greedy")
    # the first call runs eagerly and captures the decoders, the second captures the weighted step
    first = [pl.train_step_scst(img, None, image_keys=["img0", "img1"], **kw)["hist"].clone() for _ in range(2)]
    torch.cuda.synchronize()
    reads = []
    for name in ("tolist", "item", "cpu"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name,
                            lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n), _o(self, *a, **k))[1])
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o3 = pl.train_step_scst(img, None, image_keys=["img0", "img1"], seed=5, **kw)
        h3 = o3["hist"].clone()
        o4 = pl.train_step_scst(img, None, image_keys=["img3", "img2"], seed=5, **kw)  # a new index: one async upload
        h4, s4, f4, r4 = o4["hist"].clone(), o4["slen"].clone(), o4["fin"].clone(), o4["rewards"]
        o5 = pl.train_step_scst(img, None, image_keys=["img3", "img2"], **kw)
        h5 = o5["hist"].clone()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert reads == [], reads
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(h3, h4) and not torch.equal(h3, h5)  # the same seed repeats; no seed draws anew
    assert not torch.equal(first[0], first[1])
    assert math.isfinite(float(o5["loss"]))
    from fpnmt.decode import sampled_ids
    # the replayed step scored what it sampled, against the images the new index names
    ids = sampled_ids(h4, s4, f4)
    want = dev.host.score(["img3", "img2"], [ids[:c["n"]], ids[c["n"]:]])
    assert np.allclose(r4.cpu().numpy().reshape(-1), want, rtol=1e-12, atol=0)
    ent = next(iter(pl.engine._wsteps.values()))
    assert len(pl.engine._wsteps) == 1 and ent[0] == 5 and ent[1] is not None


def test_plain_host_and_device_reward_steps_alternate_on_one_engine(tables):
    """D P D H P D P on a graph engine (each kind captured once, then replayed
    in turn) leaves the arena of the same sequence run eagerly, bit for bit;
    the host-reward and the device-reward step share ONE captured weighted
    step, and train_step's graphs are the ones captured first."""
    dev, corpus = tables
    c = SC
    keys = ["img2", "img5"]
    refs = [corpus[k] for k in keys]
    E, G = _pipe(35, 1e-4, False), _pipe(35, 1e-4, True)
    g = torch.Generator().manual_seed(3)
    plain_tok = torch.randint(4, c["vocab"], (c["B"], c["T"]), generator=g)
    plain_tok[:, 0], plain_tok[:, -1] = 2, 3
    plain_tok = plain_tok.to(DEV)
    seen = {}
    for i, kind in enumerate("DPDHPDP"):
        img = _images(c["B"], c["image"], 40 + i)
        for pl in (E, G):
            if kind == "P":
                loss = pl.train_step(img, plain_tok)
            elif kind == "H":
                loss = pl.train_step_scst(img, refs, n_samples=c["n"], seed=i)["loss"]
            else:
                loss = pl.train_step_scst(img, None, n_samples=c["n"], reward=dev, image_keys=keys, seed=i)["loss"]
        assert math.isfinite(float(loss))
        if G.engine.graphs is not None:
            assert seen.setdefault("plain", G.engine.graphs) is G.engine.graphs
        ent = next(iter(G.engine._wsteps.values()))
        if ent[1] is not None:
            assert seen.setdefault("weighted", ent[1]) is ent[1]
    torch.cuda.synchronize()
    assert len(G.engine._wsteps) == 1 and "plain" in seen and "weighted" in seen
    assert int(G.engine.arena.step) == 7
    for nme in STATE:
        assert torch.equal(getattr(E.engine.arena, nme), getattr(G.engine.arena, nme)), nme


def test_interface_errors_and_the_per_batch_mode(tables):
    from fpnmt.cider_device import DeviceCiderD
    from fpnmt.decode import sampled_ids
    from utils.cider_reward import CiderDReward
    dev, corpus = tables
    c = SC
    img = _images(c["B"], c["image"], 11)
    pl = _pipe(37, 0.0, False)
    kw = dict(n_samples=c["n"])
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, reward=DeviceCiderD.from_corpus(corpus, "cpu", max_len=16), **kw)
    with pytest.raises(ValueError):  # max_seq_len - 1 = 9 > max_len
        pl.train_step_scst(img, None, reward=DeviceCiderD.from_corpus(corpus, DEV, max_len=8), **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, reward=dev, image_keys=["img0"], **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, reward=dev, image_keys=["img0", "nope"], **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, reward="device", **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, None, reward="host", **kw)
    with pytest.raises(ValueError):
        pl.train_step_scst(img, [corpus["img0"], corpus["img1"]], image_keys=["img0", "img1"], **kw)
    assert int(pl.engine.arena.step) == 0  # every error came before the step
    # image_keys None: table rows 0 .. B - 1
    a = pl.train_step_scst(img, None, reward=dev, seed=2, **kw)
    b = pl.train_step_scst(img, None, reward=dev, image_keys=["img0", "img1"], seed=2, **kw)
    assert torch.equal(a["rewards"], b["rewards"]) and torch.equal(a["loss"], b["loss"])
    # reward="device": tables of this batch's references, the document frequencies of reward=None
    refs = [corpus["img3"], corpus["img4"]]
    d = pl.train_step_scst(img, refs, reward="device", seed=2, **kw)
    ids = sampled_ids(d["hist"], d["slen"], d["fin"])
    want = CiderDReward.from_corpus(refs).score([0, 1], [ids[:3], ids[3:]])
    assert np.allclose(d["rewards"].cpu().numpy().reshape(-1), want, rtol=1e-12, atol=0)
    h = pl.train_step_scst(img, refs, seed=2, **kw)  # the host path on the same draws
    assert [s[0] for per in h["samples"] for s in per] == ids
    assert abs(h["reward_mean"] - float(d["reward_mean"])) <= 1e-12 * max(1.0, h["reward_mean"])
