"""Scene cuts as lists of frame indices: the detection rule, the check and the split into scenes.  Host arithmetic; torch only."""
import torch


def find_scene_cuts(scores, threshold=0.25, min_scene=16):
    """The cut rule over a clip's ``scene_scores`` (a tensor on either side, an array or a sequence; host arithmetic): the sorted indices t,
    1 <= t < T, at which a new scene starts.  t is a cut if ``score[t] > threshold`` and t lies at least ``min_scene`` frames after the
    previous accepted cut (or after frame 0); a candidate closer than that is dropped and does not restart the count (a photo flash gives two
    high scores a frame or two apart, and one cut at most).  The rule is causal -- nothing after t is read -- so run_video can apply it
    chunk by chunk while the clip is still uploading."""
    if isinstance(scores, torch.Tensor):
        scores = scores.detach().to("cpu", torch.float32).tolist()
    return _cut_rule(scores, 0, 0, threshold, min_scene)


def _cut_rule(scores, start, last, threshold, min_scene):
    """find_scene_cuts' rule over the scores of frames start, start + 1, ..., continued from ``last``, the previous accepted cut (0: none):
    the cuts among those frames."""
    cuts = []
    for t, v in enumerate(scores, start):
        if t >= 1 and float(v) > threshold and t - last >= min_scene:
            cuts.append(t)
            last = t
    return cuts


def _check_cuts(cuts, n, what):
    """scene_cuts as a list of ints: sorted, unique, within 1 .. n-1 (ValueError otherwise)."""
    if isinstance(cuts, torch.Tensor):
        cuts = cuts.tolist()
    try:
        cuts = [int(c) for c in cuts]
    except (TypeError, ValueError):
        raise ValueError("%s: scene_cuts must be a sequence of frame indices" % what) from None
    if any(not 1 <= c < n for c in cuts) or any(c2 <= c1 for c1, c2 in zip(cuts, cuts[1:])):
        raise ValueError("%s: scene_cuts must be sorted, unique and within 1 .. %d, got %r" % (what, n - 1, cuts))
    return cuts


def _cut_list(cuts, n, what):
    """scene_cuts as the wrappers take them -- None, empty, a tensor or a sequence -- as a checked list; [] is one scene."""
    return _check_cuts(cuts, n, what) if cuts is not None and len(cuts) else []


def _scenes(n, cuts, start=0):
    """The scenes [a, b) that the cuts split start .. n into (a cut outside that range splits nothing)."""
    edges = [start] + [c for c in cuts if start < c < n] + [n]
    return list(zip(edges[:-1], edges[1:]))
