"""Host dispatch pinned (no GPU): for a fixed list of encoder descriptors, flow dims and switch settings the library answers every
host-only query - which forward kernel, bias_part rows, bf16 gradient stash, fp16 gate stash, compact dgi, the walks' planes and
reverse-walk predicates, the per-frame drivers' plan, every *_floats size - exactly as the commit named in tests/host_dispatch_expected.py did, where each switch
setting was recorded in a fresh process (tools/record_host_dispatch.py). Here the switches change inside ONE process: equal answers also
show that no switch is cached at its first read."""
import importlib.util
import os

import pytest

import host_dispatch_expected as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_host_dispatch", os.path.join(ROOT, "tools", "record_host_dispatch.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def _set(monkeypatch, switches):
    for k in rec.SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)


def _lib():
    from lets_face_it_amd import _lib
    return _lib.lib()


def test_recorded_table_is_of_the_recorders_cases():
    """The table holds the recorder's descriptors, queries and switch settings (a recorder edited without re-recording would compare
    answers to the wrong rows)."""
    assert E.SWITCHES == rec.SWITCHES and E.ENC_QUERIES == rec.ENC_QUERIES and E.FLOW_QUERIES == rec.FLOW_QUERIES
    assert E.ENC_DESCS == rec.enc_descs() and E.FLOW_DIMS == rec.flow_dims()
    assert len(E.EXPECTED) == len(E.SWITCHES)
    for row in E.EXPECTED:
        assert len(row["enc"]) == len(E.ENC_DESCS) and len(row["flow"]) == len(E.FLOW_DIMS)


@pytest.mark.parametrize("i", range(len(E.SWITCHES)), ids=[",".join("%s=%s" % kv for kv in s.items()) or "default" for s in E.SWITCHES])
def test_host_queries_answer_as_recorded(monkeypatch, i):
    L = _lib()
    # the default setting first, then this one: a switch cached at its first read would keep the default's answer
    _set(monkeypatch, {})
    rec.answers(L)
    _set(monkeypatch, E.SWITCHES[i])
    got = rec.answers(L)
    wrong = []
    for kind, cases, queries in (("enc", E.ENC_DESCS, E.ENC_QUERIES), ("flow", E.FLOW_DIMS, E.FLOW_QUERIES)):
        for (name, desc), g, w in zip(cases, got[kind], E.EXPECTED[i][kind]):
            wrong += ["%s %s %s: %s, recorded %s" % (kind, name, q, a, b) for q, a, b in zip(queries, g, w) if a != b]
    assert not wrong, "\n".join(wrong)


def test_wide_switches_flipped_mid_process_agree_with_a_fresh_process(monkeypatch):
    """LFI_ENC_WIDE and LFI_ENC_WIDE_BWD used to be cached by the launchers and read afresh by the size queries. Flipped back and forth
    inside one process, lfi_encode_windows_stash_f16_ok and lfi_encode_windows_fwd_variant (and the other encoder queries) answer as a
    fresh process under each setting does."""
    L = _lib()
    f16 = E.ENC_QUERIES.index("stash_f16_ok")
    variants = [E.ENC_QUERIES.index(q) for q in E.ENC_QUERIES if q.startswith("fwd_variant")]
    differs = set()
    for sw in ({}, {"LFI_ENC_WIDE": "0"}, {}, {"LFI_ENC_WIDE_BWD": "0"}, {}, {"LFI_ENC_WIDE_BWD": "0"}, {"LFI_ENC_WIDE": "0"}, {}):
        _set(monkeypatch, sw)
        want = E.EXPECTED[E.SWITCHES.index(sw)]["enc"]
        for (name, desc), w, d in zip(E.ENC_DESCS, want, E.EXPECTED[0]["enc"]):
            g = rec.enc_answers(L, desc)
            assert g == w, "%s under %s: %s, a fresh process answers %s (%s)" % (name, sw or "defaults", g, w, E.ENC_QUERIES)
            if w[f16] != d[f16]:
                differs.add(("f16",) + tuple(sw))
            if any(w[v] != d[v] for v in variants):
                differs.add(("variant",) + tuple(sw))
    # the check has teeth: each switch changes the recorded answer of at least one descriptor
    assert ("f16", "LFI_ENC_WIDE") in differs and ("f16", "LFI_ENC_WIDE_BWD") in differs and ("variant", "LFI_ENC_WIDE") in differs


def test_frame_plan_switches_flipped_mid_process_agree_with_a_fresh_process(monkeypatch):
    """lfi_flow_frame_plan - what every per-frame driver of a sampler or a streaming session decides from dims and switches - reads its
    four switches at the call: flipped back and forth inside one process it answers as a fresh process under each setting does, and
    each switch changes the recorded plan of at least one descriptor. The forward cells' three fp16 products (bit 16) are recorded for
    per-frame arithmetic 9 alone: at 5, the range guard's fallback, an observed frame beyond fp16's range would leave NaN in h / c."""
    L = _lib()
    plan = E.FLOW_QUERIES.index("frame_plan")
    flips = ({"LFI_SAMPLE_CHAIN": "0"}, {"LFI_SAMPLE_WFRAG16": "0"}, {"LFI_FLOW_GENERIC": "1"}, {"LFI_PIPE_X3": "0"})
    differs = set()
    for sw in ({},) + flips + ({},) + flips[::-1] + ({},):
        _set(monkeypatch, sw)
        want = E.EXPECTED[E.SWITCHES.index(sw)]["flow"]
        for (name, dims), w, d in zip(E.FLOW_DIMS, want, E.EXPECTED[0]["flow"]):
            g = rec.flow_answers(L, dims)[plan]
            assert g == w[plan], "%s under %s: %#x, a fresh process answers %#x" % (name, sw or "defaults", g, w[plan])
            if w[plan] != d[plan]:
                differs.update(sw)
    assert differs == {k for sw in flips for k in sw}
    for row in E.EXPECTED:
        for (name, dims), w in zip(E.FLOW_DIMS, row["flow"]):
            assert not (w[plan] & 16) or (dims[-1] & 0xff) == 9, "%s: forward three-product cells recorded" % name
    assert any(w[plan] & 16 for w in E.EXPECTED[0]["flow"])     # (and the bit is recorded somewhere: the rule is exercised)
