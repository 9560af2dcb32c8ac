"""ops.view_plan without a GPU: the geometry of the training views is derived in one place; here it is held against the
composition it restates -- draw_len = stretch_input_len(speed_input_len(clip, hi_v), hi_s), pads from speed_pad and
stretch_pad -- against what a GPUTransformNeuralfp of the same configuration reports, and against the values the speed
and stretch tests pin."""
import pytest

from grafp_amd import ops
from grafp_amd.modules.transformations import GPUTransformNeuralfp
from grafp_amd.util import load_config

FIELDS = ("speed", "stretch", "clip", "speed_pad", "speed_len", "stretch_pad", "pad", "draw_len")


def _cfg(**kw):
    return dict(load_config(), **kw)


def _keys(speed_hi=None, stretch_hi=None):
    kw = {}
    if speed_hi is not None:
        kw.update(speed_prob=0.5, speed_range=[min(0.94, speed_hi), speed_hi])
    if stretch_hi is not None:
        kw.update(stretch_prob=0.7, stretch_range=[min(0.9, stretch_hi), stretch_hi])
    return kw


CASES = [(None, None), (1.06, None), (None, 1.06), (1.0, 1.0), (1.06, 1.06), (2.0, 2.0), (2.0, 1.0), (1.06, 2.0)]


@pytest.mark.parametrize("dur", (1.0, 0.1))
@pytest.mark.parametrize("speed_hi,stretch_hi", CASES)
def test_plan_is_the_composition_and_what_the_transform_reports(speed_hi, stretch_hi, dur):
    cfg = _cfg(dur=dur, **_keys(speed_hi, stretch_hi))
    p = ops.view_plan(cfg)
    clip = int(cfg["fs"] * dur)
    assert p.clip == clip
    assert p.speed == (None if speed_hi is None else (0.5, min(0.94, speed_hi), speed_hi)) == ops.speed_config(cfg)
    assert p.stretch == (None if stretch_hi is None else (0.7, min(0.9, stretch_hi), stretch_hi)) == ops.stretch_config(cfg)
    speed_len = clip if speed_hi is None else ops.speed_input_len(clip, speed_hi)
    draw_len = speed_len if stretch_hi is None else ops.stretch_input_len(speed_len, stretch_hi)
    speed_pad = 0 if speed_hi is None else ops.speed_pad(speed_hi)
    stretch_pad = 0 if stretch_hi is None else ops.stretch_pad(stretch_hi)
    assert (p.speed_pad, p.speed_len, p.stretch_pad, p.pad, p.draw_len) == (speed_pad, speed_len, stretch_pad,
                                                                           stretch_pad + speed_pad, draw_len)
    assert p.on == " and ".join(n for n, hi in (("stretch", stretch_hi), ("speed", speed_hi)) if hi is not None)
    t = GPUTransformNeuralfp(cfg, None, None, train=True)
    assert tuple(getattr(t, f) for f in FIELDS) == tuple(getattr(p, f) for f in FIELDS)


def test_pinned_values_of_the_shipped_clip():
    p = ops.view_plan(_cfg(**_keys(speed_hi=1.06)))
    assert (p.speed_pad, p.draw_len) == (8, 16976) and (p.stretch, p.stretch_pad, p.pad, p.speed_len) == (None, 0, 8, 16976)
    p = ops.view_plan(_cfg(**_keys(stretch_hi=1.06)))
    assert (p.stretch_pad, p.draw_len) == (401, 17867) and (p.speed, p.speed_pad, p.pad, p.speed_len) == (None, 0, 401, 16000)
    p = ops.view_plan(_cfg(**_keys(1.06, 1.06)))
    assert (p.stretch_pad, p.speed_pad, p.pad, p.speed_len, p.draw_len) == (401, 8, 409, 16976, 18952)
    assert p.on == "stretch and speed"
    p = ops.view_plan(_cfg())
    assert (p.speed, p.stretch, p.clip, p.speed_pad, p.speed_len, p.stretch_pad, p.pad, p.draw_len, p.on) == (
        None, None, 16000, 0, 16000, 0, 0, 16000, "")


def test_off_without_dur_has_no_clip():
    cfg = _cfg()
    del cfg["dur"]
    for extra in ({}, {"speed_prob": 0.0, "speed_range": [0.94, 1.06]}, {"stretch_range": [0.94, 1.06]}):
        p = ops.view_plan(dict(cfg, **extra))
        assert (p.clip, p.speed_len, p.draw_len, p.pad, p.on) == (None, None, None, 0, "")
        t = GPUTransformNeuralfp(dict(cfg, **extra), None, None, train=True)
        assert tuple(getattr(t, f) for f in FIELDS) == tuple(getattr(p, f) for f in FIELDS)
    with pytest.raises(KeyError, match="dur"):              # on, the clip is needed
        ops.view_plan(dict(cfg, **_keys(speed_hi=1.06)))


@pytest.mark.parametrize("key", ("speed", "stretch"))
@pytest.mark.parametrize("bad,named", (({"prob": 1.5, "range": [0.9, 1.1]}, "prob"), ({"prob": 0.5}, "range"),
                                       ({"prob": 0.5, "range": [0.4, 1.0]}, "range"), ({"range": [1.1, 1.0]}, "range"),
                                       ({"prob": 0.0, "range": "fast"}, "range")))
def test_a_bad_key_of_either_pair_is_refused_with_its_name(key, bad, named):
    other = "stretch" if key == "speed" else "speed"
    good = {f"{other}_prob": 1.0, f"{other}_range": [0.94, 1.06]}
    with pytest.raises(ValueError, match=f"{key}_{named}"):
        ops.view_plan(_cfg(**good, **{f"{key}_{k}": v for k, v in bad.items()}))
