"""Ensemble decoding (BeamDecoder / SampleDecoder / Pipeline.predict_batch with
ensemble=...): the decoders against a literal CPU ensemble search on the
oracle's models (tests/ensemble_ref.py), a model ensembled with itself, sample
mode against the oracle's teacher-forced log-probabilities, constraints on the
combined row, graph replay, Pipeline.load_member, and the error paths."""
import pytest
import torch

from constrain_ref import constrain_ref
from ensemble_ref import cpu_ensemble_beam_search, cpu_sequence_logp, normalise
from test_gpu_beam_search import C_CFG, _pipeline, cpu_beam_search, cpu_nbest
from test_gpu_constrained_decode import violates

pytestmark = pytest.mark.gpu

DEV = "cuda"

# The members, chosen on the CPU oracle before any GPU run. The main model is C_CFG's (seed 13, 2 layers,
# end_bias 3.0); alone, its best caption is the empty one on all three images, and with members that also carry
# the <end> bias so is nearly every ensemble's (members of seeds 21-28 and 100-143 were tried: no pair met the
# second condition in all four cases). The members therefore have no <end> bias: alone they never end ("a":
# 23 / 46 repeated, "b": 172 repeated) and the ensembles settle on captions of their own (105 / 122 / 179 / 39
# runs). Of seeds 21-32, 40-54 and 60-74 for "a" only 72 met both conditions with equal weights in both modes; of
# the unequal weights tried for it, (3, 4) did in both modes. Of seeds 80-89 for "b", 83 did for equal weights
# and (1, 2, 3). Smallest (step margin, key gap) over the three images in the CPU search, all above 1e-3:
#   a  prob    equal (1.18e-2, 1.10e-3)  unequal (9.16e-3, 2.98e-3)   logprob equal (1.94e-3, 1.43e-3)  unequal (1.20e-3, 1.41e-3)
#   ab prob    equal (3.83e-3, 7.16e-3)  unequal (1.25e-3, 4.06e-3)    logprob equal (2.27e-3, 1.19e-3)  unequal (2.02e-3, 1.17e-3)
#   The ensemble's best caption differs from every member's own on 1-3 images in every case.
# The constrained case uses "a", "prob", (3, 4): margins (4.71e-3, 8.77e-3); with equal weights the CPU search has a
# step margin of 2.5e-4 on image 1, too thin to compare ids.
MEMBERS = {"a": dict(seed=72, n_layers=2, end_bias=0.0), "b": dict(seed=83, n_layers=1, end_bias=0.0)}
SETS = {"a": ("a",), "ab": ("a", "b")}
WEIGHTS = {"a": {"equal": None, "unequal": (3.0, 4.0)}, "ab": {"equal": None, "unequal": (1.0, 2.0, 3.0)}}


def _oracle(pl, n_layers, imgs):
    from oracle import ref_cpu as R
    sd = {k: v.detach().float().cpu().clone() for k, v in pl.transformer.state_dict().items()}
    cfg = dict(num_layers=n_layers, num_heads=8, backbone="resnet50")
    encs = [R.encoder(sd, imgs[i][None], cfg) for i in range(imgs.shape[0])]
    return dict(sd=sd, cfg=cfg, encs=encs)


@pytest.fixture(scope="module")
def models():
    """The main model and the two members on the GPU, each one's weights,
    config and encoder outputs for the CPU oracle, and each one's best
    caption decoded alone on the CPU (computed once)."""
    import fpnmt
    c = C_CFG
    fpnmt.set_precision("fp32")
    imgs = torch.rand(c["n_img"], c["image"], c["image"], 3, generator=torch.Generator().manual_seed(c["image_seed"])) * 2 - 1
    pls = {"main": _pipeline(c["n_layers"], c["vocab"], c["image"], c["model_seed"], c["T"], c["end_bias"])}
    layers = {"main": c["n_layers"]}
    for name, m in MEMBERS.items():
        pls[name] = _pipeline(m["n_layers"], c["vocab"], c["image"], m["seed"], c["T"], m["end_bias"])
        layers[name] = m["n_layers"]
    ora = {k: _oracle(pls[k], layers[k], imgs) for k in pls}
    pl = pls["main"]
    for k, o in ora.items():
        o["alone"] = [cpu_nbest(*cpu_beam_search(o["sd"], o["cfg"], o["encs"][i], c["T"], c["K"], pl.start_token,
                                                 pl.end_token)[:4], 0.0)[0][0][0] for i in range(c["n_img"])]
    return dict(pl=pl, pls=pls, ora=ora, imgs=imgs, cache={})


def _members(m, which):
    return [m["pls"][k].transformer for k in SETS[which]]


def _oracles(m, which):
    return [m["ora"]["main"]] + [m["ora"][k] for k in SETS[which]]


def _cpu_search(m, which, mode, wname, constrain=None):
    key = (which, mode, wname, constrain is not None)
    if key not in m["cache"]:
        c, pl = C_CFG, m["pl"]
        ora = _oracles(m, which)
        w = normalise(WEIGHTS[which][wname], len(ora))
        m["cache"][key] = [cpu_ensemble_beam_search(ora, i, c["T"], c["K"], pl.start_token, pl.end_token, w, mode,
                                                    constrain) for i in range(c["n_img"])]
    return m["cache"][key]


@pytest.mark.parametrize("wname", ["equal", "unequal"])
@pytest.mark.parametrize("mode", ["prob", "logprob"])
@pytest.mark.parametrize("which", ["a", "ab"])
def test_decoder_matches_cpu_ensemble_beam_search_fp32(models, which, mode, wname):
    """All n-best id lists == the literal CPU ensemble search, scores within
    the project's fp32 logit bound (1e-3) per token. Conditions on the
    inputs: the CPU search's step margin and key gap exceed that bound on
    every image, and on some image the ensemble's best caption is not the
    best caption of any member decoded alone (else the test could not tell an
    ensemble from its first member)."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl = m["pl"]
    got = pl.predict_batch(m["imgs"].to(DEV), c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"],
                           ensemble=_members(m, which), ensemble_mode=mode, ensemble_weights=WEIGHTS[which][wname])
    differs = False
    for i in range(c["n_img"]):
        seqs, score, blen, fin, margin = _cpu_search(m, which, mode, wname)[i]
        ref, gap = cpu_nbest(seqs, score, blen, fin, 0.0)
        alone = [o["alone"][i] for o in _oracles(m, which)]
        differs = differs or all(ref[0][0] != a for a in alone)
        print(f"{which} {mode} {wname} image {i}: step margin {margin:.3e}, key gap {gap:.3e}, best {ref[0][0]}, "
              f"members alone {alone}")
        assert margin > 1e-3 and gap > 1e-3, (i, margin, gap)
        assert [ids for ids, _ in got[i]] == [ids for ids, _, _ in ref], (i, got[i], ref)
        for (_, s), (_, r, n) in zip(got[i], ref):
            assert abs(s - r) <= 1e-3 * max(n, 1), (i, s, r, n)
    assert differs, "the ensemble's best caption is a member's own on every image"


def test_model_with_itself(models):
    """ensemble=[the model itself], "logprob": the geometric mean of a
    distribution with itself is that distribution, so the n-best ids are the
    plain decode's and the scores agree to 1e-3 per token; crossed caches or
    row tables would show. The same for mode="reference"."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    kw = dict(beam_n=c["K"], use_graph=False)
    ens = dict(ensemble=[pl.transformer], ensemble_mode="logprob")
    plain = pl.predict_batch(imgs, c["T"], mode="beam", n_best=c["K"], **kw)
    both = pl.predict_batch(imgs, c["T"], mode="beam", n_best=c["K"], **kw, **ens)
    for i in range(c["n_img"]):
        assert [ids for ids, _ in both[i]] == [ids for ids, _ in plain[i]], (i, both[i], plain[i])
        for (ids, s), (_, r) in zip(both[i], plain[i]):
            assert abs(s - r) <= 1e-3 * (len(ids) + 1), (i, s, r)
    assert pl.predict_batch(imgs, c["T"], mode="reference", **kw, **ens) == pl.predict_batch(imgs, c["T"], **kw)


@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_sample_mode_scores_are_the_combined_log_probability(models, mode):
    """Every drawn (ids, logp): the oracle's teacher-forced log-probability
    of ids under the combined distribution is within 1e-3 per token; the
    same seed repeats the draws."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    kw = dict(use_graph=False, mode="sample", n_samples=4, seed=11, ensemble=_members(m, "a"), ensemble_mode=mode,
              ensemble_weights=WEIGHTS["a"]["unequal"])
    got = pl.predict_batch(imgs, c["T"], **kw)
    assert got == pl.predict_batch(imgs, c["T"], **kw)
    assert got != pl.predict_batch(imgs, c["T"], **dict(kw, seed=12))
    w = normalise(WEIGHTS["a"]["unequal"], 2)
    memo = {}
    for i in range(c["n_img"]):
        for ids, logp in got[i]:
            key = (i, tuple(ids))
            if key not in memo:
                memo[key] = cpu_sequence_logp(_oracles(m, "a"), i, ids, len(ids) < c["T"], pl.start_token,
                                              pl.end_token, w, mode)
            want, n = memo[key]
            assert abs(logp - want) <= 1e-3 * n, (i, ids, logp, want)


CONS = dict(no_repeat_ngram=2, min_len=3)


def test_constraints_apply_to_the_combined_row(models):
    """no_repeat_ngram 2 and min_len 3 on the two-model ensemble: no caption
    repeats a bigram or is shorter than 3, and the ids are the CPU ensemble
    search's with constrain_ref applied to the combined row."""
    import fpnmt
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl = m["pl"]
    end = pl.end_token
    got = pl.predict_batch(m["imgs"].to(DEV), c["T"], beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"],
                           ensemble=_members(m, "a"), ensemble_weights=WEIGHTS["a"]["unequal"], **CONS)
    cons = dict(CONS, repetition_penalty=1.0, banned_tokens=())
    rule = lambda row, seq, t: constrain_ref(row, seq, t, 0, 2, 1.0, 3, end, ())  # noqa: E731
    for i in range(c["n_img"]):
        seqs, score, blen, fin, margin = _cpu_search(m, "a", "prob", "unequal", rule)[i]
        ref, gap = cpu_nbest(seqs, score, blen, fin, 0.0)
        print(f"constrained image {i}: step margin {margin:.3e}, key gap {gap:.3e}")
        assert margin > 1e-3 and gap > 1e-3, (i, margin, gap)
        assert [ids for ids, _ in got[i]] == [ids for ids, _, _ in ref], (i, got[i], ref)
        for ids, _ in got[i]:
            assert violates(ids, c["T"], pl.start_token, cons) is None, (i, ids)


def test_ensemble_decode_graph_matches_eager_bf16():
    """Eager == captured graphs == a second replay for the two-model
    ensemble, ids and bitwise equal scores, beam and sample mode, and the
    result is not the main model's own."""
    import fpnmt
    fpnmt.set_precision("bf16")
    try:
        T, vocab, image, n_img = 12, 300, 224, 3
        pl = _pipeline(2, vocab, image, 17, T, end_bias=3.2)
        other = _pipeline(1, vocab, image, 18, T, end_bias=1.0)
        g = torch.Generator().manual_seed(6)
        imgs = (torch.rand(n_img, image, image, 3, generator=g) * 2 - 1).to(DEV)
        ens = dict(ensemble=[other], ensemble_mode="logprob", ensemble_weights=(1.0, 3.0))
        for kw in (dict(beam_n=4, mode="beam", n_best=4), dict(mode="sample", n_samples=6, top_p=0.9, seed=31)):
            a = pl.predict_batch(imgs, T, use_graph=False, **kw, **ens)
            b = pl.predict_batch(imgs, T, use_graph=True, **kw, **ens)
            c = pl.predict_batch(imgs, T, use_graph=True, **kw, **ens)  # replay of the captured graphs
            assert a == b == c, kw
            assert a != pl.predict_batch(imgs, T, use_graph=True, **kw), kw
    finally:
        fpnmt.set_precision("fp32")


def test_load_member(models, tmp_path, monkeypatch):
    """A checkpoint written by a pipeline, loaded as a bare Transformer
    without an engine, decodes in an ensemble exactly as the original
    Transformer object does as the member."""
    import fpnmt
    from fpnmt import train
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    src = m["pls"]["b"]  # one layer: the architecture argument is needed
    path = str(tmp_path / "member.safetensors")
    src.ckpt.write(path)
    made = []
    real = train.TrainEngine.__init__
    monkeypatch.setattr(train.TrainEngine, "__init__", lambda self, *a, **k: (made.append(1), real(self, *a, **k))[1])
    member = pl.load_member(path, n_layers=MEMBERS["b"]["n_layers"])
    assert not made, "load_member built a TrainEngine"
    assert member is not src.transformer
    for a, b in zip(member.state_dict().values(), src.transformer.state_dict().values()):
        assert torch.equal(a, b)
    kw = dict(beam_n=c["K"], use_graph=False, mode="beam", n_best=c["K"], ensemble_mode="prob")
    loaded = pl.predict_batch(imgs, c["T"], ensemble=[member], **kw)
    direct = pl.predict_batch(imgs, c["T"], ensemble=[src], **kw)  # a Pipeline: its .transformer is taken
    assert loaded == direct
    assert loaded != pl.predict_batch(imgs, c["T"], **{k: v for k, v in kw.items() if k != "ensemble_mode"})
    with pytest.raises((KeyError, ValueError)):
        pl.load_member(path)  # this pipeline's two layers: the checkpoint has one


def test_nothing_changes_without_an_ensemble(models, monkeypatch):
    """No ensemble: the decoder is created under the key it always had, holds
    a single model record and makes no fpnmt_logits_ensemble call. With one:
    a key of its own, one call per position between the last member's logits
    and the step kernel, and strong references to the members."""
    import fpnmt
    from fpnmt import decode as D
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    names = []
    real = D.call
    monkeypatch.setattr(D, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    pl.__dict__.pop("_decoders", None)
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam")
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False)
    pl.predict_batch(imgs, c["T"], use_graph=False, mode="sample", n_samples=2, seed=1)
    assert set(pl._decoders) == {(c["n_img"], c["K"], c["T"], False, "beam", 0.0),
                                 (c["n_img"], c["K"], c["T"], False, "reference", 0.0),
                                 (c["n_img"], 2, c["T"], False, "sample", 1.0, 0, 1.0, 0, 1.0, 0, ())}
    assert all(len(d.models) == 1 and d.models[0].tr is pl.transformer for d in pl._decoders.values())
    assert "fpnmt_logits_ensemble" not in names and "fpnmt_beam_step_log" in names
    del names[:]
    members = _members(m, "ab")
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", ensemble=members)
    assert len(pl._decoders) == 4
    dec = [d for d in pl._decoders.values() if len(d.models) == 3][0]
    assert [r.tr for r in dec.models] == [pl.transformer] + members
    assert [r.L for r in dec.models] == [2, 2, 1] and dec.models[0].kv is not dec.models[1].kv
    assert names.count("fpnmt_logits_ensemble") == names.count("fpnmt_beam_step_log") == c["T"]
    assert names.count("fpnmt_embed_posenc_fwd") == 3 * c["T"]
    i = names.index("fpnmt_logits_ensemble")
    assert names[i + 1] == "fpnmt_beam_step_log" and names[i - 1] == "fpnmt_decode_attention"
    # the same members, mode and weights: the same decoder; other weights: another
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", ensemble=members,
                     ensemble_weights=(1, 1, 1))
    assert len(pl._decoders) == 4
    pl.predict_batch(imgs, c["T"], beam_n=c["K"], use_graph=False, mode="beam", ensemble=members,
                     ensemble_weights=(2, 1, 1))
    assert len(pl._decoders) == 5


def test_ensemble_arguments_are_validated(models):
    import fpnmt
    from fpnmt import _lib as L
    from fpnmt.decode import BeamDecoder, SampleDecoder
    fpnmt.set_precision("fp32")
    m, c = models, C_CFG
    pl, imgs = m["pl"], m["imgs"].to(DEV)
    a = m["pls"]["a"].transformer
    kw = dict(beam_n=c["K"], use_graph=False, mode="beam")
    for bad, word in ((dict(ensemble=[a] * L.ENSEMBLE_MAX), f"got {L.ENSEMBLE_MAX + 1}"),
                      (dict(ensemble=[a], ensemble_mode="mean"), "'mean'"),
                      (dict(ensemble=[a], ensemble_weights=(1.0,)), "1 weights"),
                      (dict(ensemble=[a], ensemble_weights=(1.0, 2.0, 3.0)), "3 weights"),
                      (dict(ensemble=[a], ensemble_weights=(1.0, 0.0)), "0.0"),
                      (dict(ensemble=[a], ensemble_weights=(1.0, -1.5)), "-1.5"),
                      (dict(ensemble=[a], ensemble_weights=(1.0, float("nan"))), "nan"),
                      (dict(ensemble=[a], ensemble_weights=(1.0, float("inf"))), "inf"),
                      (dict(ensemble_mode="logprob"), "'logprob'"),
                      (dict(ensemble_weights=(1.0,)), "(1.0,)"),
                      (dict(ensemble=[object()]), "not a Transformer")):
        for mode_kw in (kw, dict(use_graph=False, mode="sample", n_samples=2)):
            with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
                pl.predict_batch(imgs, c["T"], **mode_kw, **bad)
    other = _pipeline(1, c["vocab"] + 1, c["image"], 5, c["T"], 0.0)  # another vocabulary
    with pytest.raises(ValueError, match=f"vocabulary {c['vocab'] + 1}"):
        pl.predict_batch(imgs, c["T"], ensemble=[other], **kw)
    short = _pipeline(1, c["vocab"], c["image"], 5, c["T"] - 2, 0.0)  # a shorter positional table
    for cls in (BeamDecoder, SampleDecoder):
        with pytest.raises(ValueError, match="positional table"):
            cls(pl.transformer, c["n_img"], 2, c["T"], pl.start_token, pl.end_token, ensemble=[short.transformer])
    pl.predict_batch(imgs, c["T"], ensemble=(), ensemble_mode="prob", ensemble_weights=None, **kw)  # the defaults
