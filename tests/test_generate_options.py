"""generate.py states every option's checks (RULES) and every option group's switch and settings (GROUPS, FIGURES) once, for the flag path
(parse_args, main) and the keyword path (generate_for_objects) alike.  CPU only and without a net: the cases of the rule tests are
searched from the table itself, so a new rule is covered without a new test."""
import inspect
import itertools
import lzma
import math
import os
import types

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import generate, mano as dmano

HERE = os.path.dirname(os.path.abspath(__file__))
SIGNATURE = inspect.signature(generate.generate_for_objects).parameters
MESH = (np.zeros((4, 3)), np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]]))
OBJS = [torch.zeros(4, 8)]

# the values a search tries for an option, by the type of its default; the first option named by a rule tries all of them
INTS, FLOATS = (-1, 0, 1, 2, 5, 6, 8, 9, 65, 1001, 1025, 4097), (-1.0, 0.0, 0.5, 1.0, 4.0, math.nan, math.inf)
FEW = {int: (0, 1, 5, 8), float: (1.0, 2.0, math.inf), bool: (False, True)}
BY_NAME = {"select_by": ("penetration", "nonsense"), "diverse_space": ("params", "nonsense"), "ttt_prior": (None, "list.json"),
           "max_self_verts": (None, -1, 0), "objects": (["a.npy"], ["a.npy", "b.npy"]), "object_indices": ([0], [0, 1])}
MESHES = {True: ([], ["a.obj"], ["a.obj", "b.obj"]), False: (None, [MESH], [MESH, MESH])}   # object_meshes: file names or (verts, faces)
# a call in which most groups are on and no rule is broken, and what turns on the group that gates a rule on the keyword path
BASE = dict(num_grasp=5, candidates=8, refine_steps=2, ttt_steps=2)
GATE = {"selection": {}, "diverse": dict(diverse_pool=6), "pushout": {}, "ttt": {}, "stability": dict(stability=True), "volume": dict(volume=True),
        "parts": dict(parts=True), "self": dict(self_collision=True), "mesh": dict(mesh_depth=True),
        "object_contact": dict(object_contact=True, object_contact_threshold=0.02)}


def flag_values(**changed):
    """The options as parse_args sees them (ho3d's defaults, its files named) plus ``rotate``."""
    o = vars(generate.build_parser("ho3d").parse_args([]))
    return {**o, "rotate": True, "objects": ["a.npy"], "object_meshes": ["a.obj"], **BASE, **changed}


def keyword_values(**changed):
    """The options as the keyword path sees them: the bound arguments of the call the tests make, and the object-side contact map off."""
    o = {k: p.default for k, p in SIGNATURE.items()}
    o.update(net=None, objs=OBJS, rotate=True, seed=0, object_indices=[0], object_meshes=[MESH], object_contact=False, object_contact_threshold=None)
    return {**o, **BASE, **changed}


def pools(rule, base, cli):
    """(option, values to try) for the options a rule reads."""
    out = []
    for i, name in enumerate(n for n in generate._rule_options(rule) if n not in ("objs", "rotate")):
        kind = type(base[name])
        values = BY_NAME.get(name) or (MESHES[cli] if name == "object_meshes" else None)
        if values is None:
            values = ({int: INTS, float: FLOATS}.get(kind, FEW[kind]) if i == 0 else FEW[kind])
        out.append((name, values))
    return out


def distance(a, b):
    """How far two assignments are apart: the options that differ, then by how much the numbers do."""
    differ = [k for k in a if repr(a[k]) != repr(b[k])]
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
    return len(differ), sum(abs(a[k] - b[k]) for k in differ if number(a[k]) and number(b[k]))


def search(rule, cli):
    """(bad, good): the values of a call that the evaluator refuses for ``rule``, and the nearest ones it accepts."""
    for rotate in (True, False):                                                   # (one rule needs objects that are not rotated)
        base = (flag_values if cli else keyword_values)(**(GATE[rule.gate] if rule.gate and not cli else {}), rotate=rotate)
        names, values = zip(*pools(rule, base, cli))
        tried = [dict(zip(names, v)) for v in itertools.product(*values)]
        verdict = [generate._broken_rule(types.SimpleNamespace(**{**base, **t}), cli) for t in tried]
        bad = next((t for t, r in zip(tried, verdict) if r is rule), None)
        if bad is not None:
            good = min((t for t, r in zip(tried, verdict) if r is None), key=lambda t: distance(bad, t))
            return {**base, **bad}, {**base, **good}
    raise AssertionError(f"{rule.names} {rule.text!r}: no value tried breaks it {'as flags' if cli else 'as keywords'}")


def argv(values):
    """(dataset, argv) of the flags that differ from the parser's defaults."""
    dataset = "ho3d" if values["rotate"] else "obman"
    default = vars(generate.build_parser(dataset).parse_args([]))
    out = []
    for k, v in values.items():
        if k in default and repr(v) != repr(default[k]):
            out += ["--" + k] + ([str(x) for x in v] if isinstance(v, list) else [str(v)])
    return dataset, out


def call(values):
    """The keyword path with no net: generate_for_objects, or generate_with_object_contact where the values turn the contact map on."""
    keywords = {k: v for k, v in values.items() if k in SIGNATURE and k not in ("net", "objs", "num_grasp", "rotate", "seed", "object_indices")}
    where, extra = generate.generate_for_objects, {}
    if values["object_contact"]:
        where, extra = generate.generate_with_object_contact, dict(object_contact_threshold=values["object_contact_threshold"])
    return where(None, values["objs"], values["num_grasp"], values["rotate"], 0, values["object_indices"], **extra, **keywords)


def rules(not_only):
    """The rules of one path, with test ids: pytest.param per rule of the table that is not marked for the other path alone."""
    return [pytest.param(r, id=f"{i}-{'-'.join(r.names)}") for i, r in enumerate(generate.RULES) if r.only != not_only]


@pytest.mark.parametrize("rule", rules("keywords"))
def test_a_broken_rule_is_refused_on_the_flag_path_and_its_nearest_good_value_passes(rule, capsys):
    bad, good = search(rule, cli=True)
    with pytest.raises(SystemExit):
        generate.parse_args(*argv(bad))
    message = capsys.readouterr().err
    assert "--" + rule.names[0] in message and "(got " in message, message
    assert generate._rule_message(rule, types.SimpleNamespace(**bad), cli=True) in message, message
    args = generate.parse_args(*argv(good))
    assert all(repr(getattr(args, k)) == repr(v) for k, v in good.items() if hasattr(args, k)), "the good values are not what was parsed"


@pytest.mark.parametrize("rule", rules("cli"))
def test_a_broken_rule_is_refused_on_the_keyword_path_before_any_work(rule):
    bad, good = search(rule, cli=False)
    assert rule.gate is None or generate.GROUPS[rule.gate].wanted(types.SimpleNamespace(**bad))
    with pytest.raises(RuntimeError, match=rule.names[0]) as e:                    # net = None: nothing may touch it
        call(bad)
    assert str(e.value) == "generate_for_objects: " + generate._rule_message(rule, types.SimpleNamespace(**bad), cli=False)
    assert "(got " in str(e.value) and "--" not in str(e.value)
    assert generate._broken_rule(types.SimpleNamespace(**good), cli=False) is None


def test_a_gate_is_read_by_the_keyword_path_only():
    """--torque_length -1 is refused without --stability; torque_length=-1 is looked at only with stability."""
    with pytest.raises(SystemExit):
        generate.parse_args("ho3d", ["--torque_length", "-1"])
    off = types.SimpleNamespace(**keyword_values(torque_length=-1.0))
    assert generate._broken_rule(off, cli=False) is None
    assert generate._broken_rule(types.SimpleNamespace(**flag_values(torque_length=-1.0)), cli=True).names == ("torque_length",)
    on = types.SimpleNamespace(**keyword_values(torque_length=-1.0, select_by="stability"))      # on with candidates and select_by, too
    assert generate._broken_rule(on, cli=False).names == ("torque_length",)
    assert {r.gate for r in generate.RULES if r.gate} <= set(generate.GROUPS) and {r.only for r in generate.RULES} == {None, "cli", "keywords"}
    # the limit on candidates is the keyword path's alone, as it has been
    assert generate.parse_args("ho3d", ["--candidates", "5000"]).candidates == 5000
    with pytest.raises(RuntimeError, match="candidates"):
        call(keyword_values(candidates=5000))


@pytest.mark.parametrize("dataset", sorted(generate.DATASETS))
def test_flags_and_keywords_share_names_and_defaults(dataset):
    flags = vars(generate.build_parser(dataset).parse_args([]))
    assert {k for k in SIGNATURE if k not in flags} == {"net", "objs", "rotate", "object_indices", "proxies"}
    for name, p in SIGNATURE.items():
        if name not in flags or p.default is inspect.Parameter.empty:              # (seed and num_grasp are positional: no default)
            continue
        if isinstance(p.default, bool):
            assert flags[name] in (0, 1) and bool(flags[name]) is p.default, name
        elif name == "object_meshes":
            assert flags[name] == [] and p.default is None
        else:
            assert repr(flags[name]) == repr(p.default), (name, flags[name], p.default)
    assert {k for k, p in SIGNATURE.items() if p.default is inspect.Parameter.empty and k in flags} == {"num_grasp", "seed"}


# every group and the options each of which alone turns it on
SWITCHES = {"selection": ["candidates"], "diverse": ["diverse_pool"], "pushout": ["refine_steps"], "spin": ["refine_spin"], "curl": ["refine_curl"],
            "ttt": ["ttt_steps"], "diversity": ["diversity"], "beam": ["beam_width"], "stability": ["stability"],
            "volume": ["volume", "max_volume"], "parts": ["parts", "min_fingers", "need_thumb"], "self": ["self_collision", "max_self_verts"],
            "mesh": ["mesh_depth", "max_mesh_depth"], "object_contact": ["object_contact"]}


def test_every_group_is_off_at_the_defaults_and_on_with_each_switch_alone():
    assert set(SWITCHES) == set(generate.GROUPS), "a group was added or removed: say here what turns it on"
    defaults = [vars(generate.build_parser(d).parse_args([])) for d in sorted(generate.DATASETS)]
    defaults.append({**{k: p.default for k, p in SIGNATURE.items()}, "object_contact": False})
    for base in defaults:
        for name, group in generate.GROUPS.items():
            assert group.wanted(types.SimpleNamespace(**base)) is False, name
            for switch in SWITCHES[name]:
                on = [g for g, other in generate.GROUPS.items() if other.wanted(types.SimpleNamespace(**{**base, switch: 1}))]
                assert on == [name], (switch, on)
            assert set(group.keywords) <= set(base) | {"object_contact_threshold"} and (group.switch is None or group.switch in SIGNATURE), name
    for fig in generate.FIGURES:
        assert [fig.switch, *fig.limits] == SWITCHES[fig.key] and generate.GROUPS[fig.key] is fig
        assert fig.limited(types.SimpleNamespace(**defaults[-1])) is False
    both = types.SimpleNamespace(**{**defaults[-1], "candidates": 8, "select_by": "stability"})    # the one group with a second way in
    assert generate.GROUPS["stability"].wanted(both) and not generate.GROUPS["stability"].wanted(types.SimpleNamespace(**{**vars(both), "candidates": 0}))


def test_the_figures_come_in_the_order_of_FIGURES(monkeypatch, tmp_path):
    """The order _Figure documents -- of launches, dict keys, JSON fields and summaries -- is FIGURES' own: the dicts of a call show
    volume, parts, self, mesh (test_generate_combined.documented_keys), and _Options.figures, which both paths of a call loop over,
    holds the active ones in that order with the settings each figure states."""
    assert [fig.key for fig in generate.FIGURES] == ["volume", "parts", "self", "mesh"]
    path = str(tmp_path / "MANO_RIGHT.pkl")
    with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    net = types.SimpleNamespace(rh_mano=types.SimpleNamespace(faces=np.asarray(dmano.read_mano_pkl(path)["faces"])))
    seen = []
    monkeypatch.setattr(generate, "plan_calls", lambda counts, rows, rows_per_call: seen.append((list(counts), rows, rows_per_call)) or [])
    made, options = [], generate._Options

    class Spy(options):
        def __init__(self, **fields):
            options.__init__(self, **fields)
            made.append(self)
    monkeypatch.setattr(generate, "_Options", Spy)
    out = generate.generate_for_objects(net, OBJS, 5, True, 3, [0], candidates=8, max_volume=2.0, volume_res=0.004, need_thumb=True, max_self_verts=1,
                                        mesh_depth=True, object_meshes=[MESH], select_by="stability", beam_width=4, beam_poses=2)
    assert out == [None] and seen == [([8], 8, 16384)]
    opt, = made
    assert [fig for fig, _ in opt.figures] == list(generate.FIGURES)
    assert [sorted(s) for _, s in opt.figures] == [["max_volume", "res"], ["min_fingers", "min_verts", "need_thumb", "table", "threshold"],
                                                   ["margin", "max_verts", "reach", "table"], ["max_depth"]]
    assert opt.figures[0][1] == dict(res=0.004, max_volume=2.0) and opt.figures[3][1] == dict(max_depth=math.inf)
    assert (opt.stability, opt.beam, opt.ttt, opt.object_contact, opt.seed, opt.candidates) == (True, (2, 4), None, None, 3, 8)
    generate.generate_with_object_contact(net, OBJS, 5, True, 3, [0], object_contact_threshold=0.03, volume=True)
    assert made[1].object_contact == 0.03 and [fig for fig, _ in made[1].figures] == [generate.FIGURES[0]] and made[1].stability is False
