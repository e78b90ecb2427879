"""Parameter groups of the training step: which tensors are trained, at which
fraction of the schedule's rate, and with how much weight decay (not in the
reference, whose one Adam updates everything at one rate, utils/pipeline.py:
29-30). Host-side model only: no GPU is needed to import or use this module.

A ParamGroup selects parameters by name prefix (names as
``transformer.named_parameters()`` gives them) or by a callable
``(name, param) -> bool``; the first group that matches a parameter owns it,
and a parameter no group matches belongs to the implicit default group
(lr_scale 1, weight_decay 0, trainable). TrainEngine(param_groups=[...])
turns assign()'s rows into the per-segment device table of
fpnmt_amsgrad_step_groups.

The usual captioning recipe:
  phase 1  cross-entropy, CNN frozen     [backbone_group(model, frozen=True)]
  phase 2  CNN at a tenth of the rate    [backbone_group(model, lr_scale=0.1)]
  phase 3  self-critical, CNN frozen     [feature_extractor_group(model, frozen=True)]
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Sequence, Union

FE_PREFIX = "encoder.feature_extractor."
DEFAULT_NAME = "default"  # the implicit group of unmatched parameters
DEFAULT_ROW = (-1, 1.0, 0.0, False)


@dataclass(frozen=True)
class ParamGroup:
    """name: the handle of TrainEngine.set_lr_scale / set_weight_decay /
    set_frozen. match: a tuple of name prefixes, or (name, param) -> bool.
    lr_scale: multiplies the schedule's rate (0 is legal: the moments advance,
    the parameter only decays). weight_decay: decoupled (AdamW) decay
    coefficient, a number or a callable (name, param) -> number such as
    decay_matrices(w). frozen: the group is neither differentiated nor
    updated."""
    name: str
    match: Union[Sequence[str], Callable]
    lr_scale: float = 1.0
    weight_decay: Union[float, Callable] = 0.0
    frozen: bool = False

    def matches(self, name, param):
        if callable(self.match):
            return bool(self.match(name, param))
        pref = (self.match,) if isinstance(self.match, str) else tuple(self.match)
        return name.startswith(pref)


def _finite_nonneg(x, what):
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {x!r}") from None
    if not (math.isfinite(v) and v >= 0.0):  # NaN fails both
        raise ValueError(f"{what} must be finite and >= 0, got {x!r}")
    return v


def decay_of(weight_decay, name, param, what="weight_decay"):
    """The decay coefficient of one tensor: weight_decay itself, or its value
    at (name, param) when it is a callable. Validated."""
    w = weight_decay(name, param) if callable(weight_decay) else weight_decay
    return _finite_nonneg(w, what)


def decay_matrices(wd):
    """weight_decay=decay_matrices(wd): wd on tensors with ndim >= 2 (conv and
    dense kernels, embeddings), none on vectors (biases, LayerNorm and
    BatchNorm gamma / beta)."""
    wd = _finite_nonneg(wd, "decay_matrices: wd")
    return lambda name, param: wd if param.ndim >= 2 else 0.0


def validate(groups):
    """The checks that need no parameter list: finite non-negative numbers,
    unique names."""
    groups = list(groups or ())
    seen = set()
    for g in groups:
        if g.name in seen:
            raise ValueError(f"param_groups: duplicate group name {g.name!r}")
        seen.add(g.name)
        _finite_nonneg(g.lr_scale, f"group {g.name!r}: lr_scale")
        if not callable(g.weight_decay):
            _finite_nonneg(g.weight_decay, f"group {g.name!r}: weight_decay")
    return groups


def assign(names, params, groups):
    """Per arena segment (names[i], params[i]) the row (group index, lr_scale,
    weight_decay, frozen): the first matching group wins, unmatched tensors
    get DEFAULT_ROW (index -1). ValueError: a negative / NaN / infinite
    lr_scale or weight_decay, duplicate group names, a group that matches no
    parameter."""
    groups = validate(groups)
    rows = []
    hits = [0] * len(groups)
    for n, p in zip(names, params):
        row = DEFAULT_ROW
        for gi, g in enumerate(groups):
            if g.matches(n, p):
                hits[gi] += 1
                row = (gi, float(g.lr_scale),
                       decay_of(g.weight_decay, n, p, f"group {g.name!r}: weight_decay of {n}"), bool(g.frozen))
                break
        rows.append(row)
    empty = [g.name for g, h in zip(groups, hits) if h == 0]
    if empty:
        raise ValueError(f"param_groups: groups that match no parameter (or only parameters an earlier group "
                         f"owns): {empty}")
    return rows


def _stage_prefixes(transformer):
    """The feature extractor's staged-backward prefixes as full parameter-name
    prefixes: [heads, FPN, backbone segments...] (FeatureExtractor.stage_prefixes)."""
    fe = transformer.encoder.feature_extractor
    return [[FE_PREFIX + p for p in ps] for ps in fe.stage_prefixes()]


def backbone_prefixes(transformer):
    """Prefixes covering encoder.feature_extractor.retinanet_model.backbone.:
    the backbone segments of the staged backward."""
    return tuple(p for ps in _stage_prefixes(transformer)[2:] for p in ps)


def feature_extractor_prefixes(transformer):
    """Prefixes covering the whole encoder.feature_extractor. (heads, FPN,
    backbone)."""
    return tuple(p for ps in _stage_prefixes(transformer) for p in ps)


def backbone_group(transformer, lr_scale=1.0, weight_decay=0.0, frozen=False, name="backbone"):
    return ParamGroup(name, backbone_prefixes(transformer), lr_scale, weight_decay, frozen)


def feature_extractor_group(transformer, lr_scale=1.0, weight_decay=0.0, frozen=False, name="feature_extractor"):
    return ParamGroup(name, feature_extractor_prefixes(transformer), lr_scale, weight_decay, frozen)


def recipe_groups(transformer, backbone_lr_scale=1.0, freeze=(), weight_decay=0.0):
    """The groups of Pipeline(backbone_lr_scale=, freeze=, weight_decay=):
    freeze is a subset of {"backbone", "feature_extractor"}; weight_decay
    applies to matrices only (decay_matrices), everywhere. Returns None when
    every argument is at its default (the engine then runs the plain step)."""
    freeze = {freeze} if isinstance(freeze, str) else set(freeze)
    bad = freeze - {"backbone", "feature_extractor"}
    if bad:
        raise ValueError(f"freeze must be a subset of {{'backbone', 'feature_extractor'}}, got {sorted(bad)}")
    s = _finite_nonneg(backbone_lr_scale, "backbone_lr_scale")
    w = _finite_nonneg(weight_decay, "weight_decay")
    if s == 1.0 and w == 0.0 and not freeze:
        return None
    wd = decay_matrices(w) if w else 0.0
    groups = [backbone_group(transformer, s, wd, bool(freeze))]
    # the rest of the feature extractor (first match wins: the backbone is taken)
    groups.append(ParamGroup("feature_extractor", feature_extractor_prefixes(transformer), 1.0, wd,
                             "feature_extractor" in freeze))
    groups.append(ParamGroup("transformer", lambda n, p: True, 1.0, wd, False))
    return groups
