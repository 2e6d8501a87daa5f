"""The conv kernel-form policy (videosd_amd/convform.py) against what it answered before it was stated once: every case of
tests/conv_form_cases.py, compared with tests/golden/conv_forms.json (recorded at the commit named there by driving HipOps on the CPU:
forms read off the descriptors, candidate lists off the calls the tuner made).  No GPU, no libvsd.so."""
import json

import pytest

import conv_form_cases as K
from videosd_amd import convform as CF
from videosd_amd import program as PR


@pytest.fixture(scope="module")
def gold():
    return json.load(open(K.GOLDEN))


@pytest.fixture(scope="module")
def committed():
    return K.committed_table()


def fstr(f):
    return "%d.%d.%d.%d" % (f[0], f[1], int(f[2] and f[1] > 1), f[3])  # (as a descriptor shows it: counters only where K is split)


def hip(mode=0, table=None, flags=None):
    ops = K.cpu_hip_ops()
    ops.tune_mode, ops.tile_override = mode, dict(table or {})
    for f in (flags or {}):
        setattr(ops, f, True)
    return ops


def test_the_case_list_is_the_fixtures(gold):
    assert [n for n, _a, _k in K.CALLS] == list(gold["resolve"]) == list(gold["candidates"]) == list(gold["keys"])
    assert len({n for n, _a, _k in K.CALLS}) == len(K.CALLS)


@pytest.mark.parametrize("name,a,kw", K.CALLS, ids=[c[0] for c in K.CALLS])
def test_key_resolved_form_and_candidates_of_a_call(gold, committed, name, a, kw):
    call = CF.conv_call(a[2], a[3], **kw)
    keys = [call.key(mode) for mode in K.MODES]
    assert json.loads(json.dumps(keys)) == gold["keys"][name]
    forms, cands = [], []
    for mode in K.MODES:
        for flags in K.FLAG_SETS:
            fl = CF.Flags(**flags)
            for _tname, table in K.table_states(keys[0], keys[1], committed):
                f = CF.resolve(call, table, mode, fl)
                forms.append(fstr(f))
                ops = hip(mode, table, flags)  # (and HipOps.conv puts that form into the descriptor)
                assert K.desc_form(ops, a, kw) == (f.tile, f.split_k, f.inkernel and f.split_k > 1, f.pipeline)
                assert ops.conv_key_of(a[2], a[3], kw) == keys[mode]
            cands.append(K.digest(CF.candidates(call, mode, fl)))
    assert " ".join(forms) == gold["resolve"][name]
    assert cands == gold["candidates"][name]


def test_a_planted_persistent_form_is_taken_by_the_call_that_fits_and_not_by_its_scaled_twin(gold):
    a, kw = K.call("taesd 64->64 32x32")
    call = CF.conv_call(a[2], a[3], **kw)
    assert len(CF.candidates(call, 0, CF.Flags())) == 111
    planted = {call.key(0): K.PLANTED["pipeline 10"]}
    assert CF.resolve(call, planted, 0, CF.Flags())[::3] == (CF.L.TILE_256x64, 10)
    scaled = CF.conv_call(a[2], a[3], out_scale=0.5)
    assert scaled.key(0) != call.key(0) and CF.resolve(scaled, planted, 0, CF.Flags()) == CF.resolve(scaled, {}, 0, CF.Flags())


@pytest.mark.parametrize("name", K.EXPLICIT_CALLS)
def test_a_call_that_names_its_form(gold, committed, name):
    a, kw = K.call(name)
    call = CF.conv_call(a[2], a[3], **kw)
    row = []
    for mode in K.MODES:
        for table in ({}, committed):
            for fkw, ink in K.EXPLICIT_FORMS:
                row.append(fstr(CF.resolve(call, table, mode, CF.Flags(), inkernel=ink, **fkw)))
                ops = hip(mode, table)
                assert fstr(K.desc_form(ops, a, dict(kw, inkernel=ink, **fkw))) == row[-1]  # (the argument ...)
                ops.inkernel_splitk = ink
                assert fstr(K.desc_form(ops, a, dict(kw, **fkw))) == row[-1]  # (... and the attribute it defaults to)
    assert " ".join(row) == gold["explicit"][name]


def test_groups_and_pairs_of_the_cases(gold, committed):
    for gname, members, split in K.GROUPS:
        calls = [K.call(m) for m in members]
        row = []
        for mode in K.MODES:
            for table in ({}, committed):
                cands = CF.group_candidates(calls, table, mode, CF.Flags(), split=split)
                row.append([list(CF.group_key(calls, split, mode)), CF.own_splits(calls, table, mode, CF.Flags()), K.digest([K.form4(f) for f in cands])])
                ops = hip(mode, table)
                assert (ops.group_key(calls, split), ops.own_splits(calls), ops.group_candidates(calls, split)) == (tuple(row[-1][0]), row[-1][1], cands)
        assert row == gold["groups"][gname], gname
    for na, nb in K.PAIRS:
        (aa, ka), (ab, kb) = K.call(na), K.call(nb)
        row = []
        for mode in K.MODES:
            for table in ({}, committed):
                shared = CF.pair_form(aa, ka, ab, kb, table, mode, CF.Flags())
                row.append([None, None] if shared is None else [shared[0], K.form4(shared[1])])
                assert hip(mode, table).pair_split(aa, ka, ab, kb) == row[-1][0]
        assert row == gold["pairs"][na + " | " + nb], (na, nb)


def pair_form_of(ops, aa, ka, ab, kb):
    shared = CF.pair_form(aa, ka, ab, kb, ops.tile_override, ops.tune_mode, CF.flags_of(ops), inkernel=ops.inkernel_splitk)
    return (None, None) if shared is None else shared


def resolved_of(ops, a, kw):
    f = CF.resolve(CF.conv_call(a[2], a[3], **kw), ops.tile_override, ops.tune_mode, CF.flags_of(ops), **{"inkernel": ops.inkernel_splitk, **CF.named_form(kw)})
    assert K.desc_form(ops, a, kw) == (f.tile, f.split_k, f.inkernel and f.split_k > 1, f.pipeline)
    return (f.tile, f.split_k, f.inkernel and f.split_k > 1, f.pipeline)


def test_every_conv_pair_and_group_call_of_the_recorded_programs(gold, committed):
    """the programs of scripts/program_fingerprint.py (the MINI network on the op emulator) under an empty table, the committed one and
    a made-up one over the program's own keys: key, resolved form, own_splits, pair_split and the members' own form, group_candidates --
    and `launches_by_kind`, asked with HipOps and with the emulator the program was recorded on (a `tile_override` and nothing else)"""
    seen = []
    for cname, prog, prog_serial in K.programs():
        seen.append(cname)
        synth = dict(K.synthetic_table(hip(), prog.calls + prog_serial.calls))
        for tname, table in (("empty", {}), ("committed", committed), ("synthetic", synth)):
            for mode in K.MODES:
                want = gold["programs"][cname][f"{tname}|{mode}"]
                ops = hip(mode, table)
                ans = [K.program_answers(ops, p.calls, resolved_of, pair_form_of) for p in (prog, prog_serial)]
                assert [K.digest(x) for x in ans] == [want["answers"], want["answers_serial"]], (cname, tname, mode)
                counted = [K.conv_launches(PR.launches_by_kind(ops, p)) for p in (prog, prog_serial)]
                assert counted == [want["launches"], want["launches_serial"]], (cname, tname, mode)
                if mode == 0:  # (the emulator has no tuning mode: alone-timed)
                    emu = prog.ops
                    emu.tile_override = table
                    assert [K.conv_launches(PR.launches_by_kind(emu, p)) for p in (prog, prog_serial)] == counted, (cname, tname)
    assert seen == list(gold["programs"])
