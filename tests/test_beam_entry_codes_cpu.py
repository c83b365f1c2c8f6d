"""The return codes of the beam search entries, case by case, against a table recorded from the commit before the host side of
csrc/ctc_beam.hip got one driver per entry family: which code an entry answers a bad call with, and which
one wins when two apply, is behaviour.

Host only.  Every argument check of these entries returns before anything is launched, and host code never dereferences a
device pointer, so the entries are called through asr._lib.lib() with a null stream and small placeholder addresses.  No listed
case expects ASR_OK or the launch code, so nothing here launches by design; a check that wrongly passes WOULD launch on an
address that is not memory, which is why the module only runs where there is no device (there it shows as a -4 mismatch).

tests/golden/beam_entry_codes.json holds rows {entry, variant, mutations, code} and is written by
`python tests/test_beam_entry_codes_cpu.py --record` with ASR_HIP_LIB pointing at a build of the commit to record from.
"""
import functools
import json
import os
import re
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entries with addresses that are not memory: no device")

TABLE = os.path.join(GOLDEN, "beam_entry_codes.json")
BAD_ARG, WORKSPACE, UNSUPPORTED, LAUNCH = -1, -2, -3, -4
T, B, V, W, K, F = 4, 1, 10, 16, 4, 8                       # frames, batch, vocabulary, beam_width, top_k, max_frames
VLM = V + 2
_PREFIX = {"ctc": "asr_ctc_beam_", "gram": "asr_gram_ctc_beam_", "gram_bias": "asr_gram_ctc_beam_bias_"}

# entry -> the variants (model, graph) it can be called in
_BOTH = ("plain", "lm", "graph", "lm+graph")
ENTRIES = {
    "asr_ctc_beam_search": ("plain",),
    "asr_ctc_beam_search_lm": ("lm",),
    "asr_ctc_beam_search_bias": ("graph", "lm+graph"),
    "asr_gram_ctc_beam_search": ("plain",),
    "asr_gram_ctc_beam_search_lm": ("lm",),
    "asr_gram_ctc_beam_search_bias": ("graph", "lm+graph"),
    "asr_ngram_score": ("lm",),
    "asr_ctx_score": ("graph",),
    "asr_ctc_beam_stream_reset": _BOTH,
    "asr_ctc_beam_stream_advance": _BOTH,
    "asr_ctc_beam_stream_result": _BOTH,
    "asr_gram_ctc_beam_stream_reset": ("plain", "lm"),
    "asr_gram_ctc_beam_stream_advance": ("plain", "lm"),
    "asr_gram_ctc_beam_stream_result": ("plain", "lm"),
    "asr_gram_ctc_beam_bias_stream_reset": _BOTH,
    "asr_gram_ctc_beam_bias_stream_advance": _BOTH,
    "asr_gram_ctc_beam_bias_stream_result": _BOTH,
}

_LM_ON = {"uni": "ptr", "vlm": VLM, "keys": "ptr", "vals": "ptr", "slots": 4, "max_probe": 2, "order": 3, "bos": V, "eos": V + 1}
_LM_OFF = {"uni": None, "vlm": 0, "keys": None, "vals": None, "slots": 0, "max_probe": 0, "order": 0, "bos": -1, "eos": -1}
_GRAPH_ON = {"g_keys": "ptr", "g_vals": "ptr", "g_slots": 4, "g_max_probe": 2, "g_ret": "ptr", "g_n_states": 3}
_GRAPH_OFF = {"g_keys": None, "g_vals": None, "g_slots": 0, "g_max_probe": 0, "g_ret": None, "g_n_states": 0}
_REST = {"stream": None, "lengths": None, "mask": None, "T": T, "Tc": T, "B": B, "V": V, "blank": 0, "beam_width": W, "top_k": K,
         "min_logp": float("-inf"), "alpha": 0.5, "beta": 0.25, "N": 2, "Lmax": 3, "finalize": 1, "Lcap": 2 * F, "max_frames": F,
         "frames_before": 0}
_OUTS_LM, _OUTS_GRAPH = ("out_ctc", "out_lm"), ("out_bias",)


@functools.lru_cache(None)
def _prototypes():
    """entry -> [(parameter name, is pointer)] from include/asr_hip.h"""
    text = open(os.path.join(ROOT, "include", "asr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(asr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        if name in ENTRIES:
            out[name] = [(a.split()[-1].lstrip("*"), "*" in a) for a in args.split(",")]
    assert sorted(out) == sorted(ENTRIES)
    return out


def _valid(entry, variant):
    """name -> value of one valid call of `entry` in `variant`; "ptr" stands for a non-null device address"""
    lm, graph = "lm" in variant, "graph" in variant
    vals = dict(_REST, **(_LM_ON if lm else _LM_OFF), **(_GRAPH_ON if graph else _GRAPH_OFF), with_lm=int(lm), with_bias=int(graph))
    call = {}
    for name, is_ptr in _prototypes()[entry]:
        if name in vals:
            call[name] = vals[name]
        elif name in ("workspace_bytes", "state_bytes"):
            call[name] = "exact"
        else:
            assert is_ptr, (entry, name)
            needed = lm or graph if name in _OUTS_LM else (graph if name in _OUTS_GRAPH else True)
            call[name] = "ptr" if needed or "stream" not in entry else None      # result takes null for the outputs it does not write
    return call


def _sizes(lib, entry, call):
    """(workspace bytes, state bytes) that `call`'s dimensions need; 0 where the dimensions are not valid"""
    family = "gram" if "gram" in entry else "ctc"
    ws = state = 0
    if "workspace_bytes" in call:
        size = "stream_workspace_bytes" if "stream" in entry else "workspace_bytes"
        ws = getattr(lib, _PREFIX[family] + size)(call.get("T", call.get("Tc")), call["B"], call["V"], call["beam_width"], call["top_k"])
    if "state_bytes" in call:
        if "with_lm" in call:                                    # reset takes the flags; advance and result go by uni and g_ret
            flags = [call["with_lm"]] + ([call["with_bias"]] if "with_bias" in call else [])
        else:
            flags = [int(call["uni"] is not None)] + ([int(call["g_ret"] is not None)] if "g_ret" in call else [])
        narrow = family == "gram" and len(flags) == 1           # the Gram-CTC entries without a graph argument
        name = _PREFIX["gram" if narrow else ("gram_bias" if family == "gram" else "ctc")] + "stream_state_bytes"
        state = getattr(lib, name)(call["B"], call["beam_width"], call["max_frames"], *flags)
    return ws, state


def run_case(lib, entry, variant, mutations):
    """the code `entry` returns for its valid call in `variant` with `mutations` (name -> value) applied.  A size is "exact" (what
    the call's own dimensions need, or the valid call's where they are not valid) or "short" (one byte less)."""
    base = _valid(entry, variant)
    call = dict(base, **mutations)
    need = [n or m for n, m in zip(_sizes(lib, entry, call), _sizes(lib, entry, base))]
    args = []
    for i, (name, _) in enumerate(_prototypes()[entry]):
        v = call[name]
        if name in ("workspace_bytes", "state_bytes"):
            v = need[name == "state_bytes"] - (v == "short")
        elif v == "ptr":
            v = 0x10000 + 0x1000 * i
        args.append(v)
    return getattr(lib, entry)(*args)


_LIMITS = ({"beam_width": 129}, {"top_k": 65}, {"beam_width": 128, "top_k": 33})          # MAX_BEAM, MAX_TOPK, MAX_EXT = 4096


def mutations_of(entry, variant):
    """every mutation of the valid call that the table tries: the single ones, then the ones that set two codes against each
    other.  A mutation that names a parameter the entry does not have, or that changes nothing, is not one."""
    base = _valid(entry, variant)
    singles = [{name: None} for name, is_ptr in _prototypes()[entry] if is_ptr]
    singles += [{d: 0} for d in ("T", "Tc", "B", "V", "beam_width", "top_k", "N", "Lmax", "Lcap", "max_frames")]
    singles += [{"blank": -1}, {"blank": V}, {"frames_before": -1}, {"frames_before": F + 1 - T}, *_LIMITS]
    singles += [{"order": 0}, {"order": 5}, {"slots": 12}, {"max_probe": 0}, {"vlm": V - 1}, {"bos": VLM}, {"eos": VLM}]
    singles += [{"g_n_states": 0}, {"g_slots": 12}, {"g_max_probe": 0}]
    singles += [{"state_bytes": "short"}, {"workspace_bytes": "short"}]
    first_out = next((n for n, _ in _prototypes()[entry] if n.startswith("out_")), "state")
    bad_arg = [{"logits": None}, {first_out: None}, {"blank": -1}]
    bad_model = [{"order": 0}, {"order": 5}, {"slots": 12}, {"vlm": V - 1}, {"bos": VLM}]
    bad_graph = [{"g_n_states": 0}, {"g_ret": None}]
    short = [{"state_bytes": "short"}, {"workspace_bytes": "short"}]
    overflow = {"frames_before": F + 1 - T}
    no_model = {"uni": None, "vlm": V - 1}                      # _lm tests vlm whatever uni is; _bias only with a model
    pairs = [dict(a, **b) for a in bad_arg + bad_model + bad_graph + [{"gram": None}] for b in _LIMITS[:2]]
    pairs += [dict(a, **b) for a in [{"gram": None}, {"top_k": 65}, overflow] for b in short]
    pairs += [dict(a, **b) for a in bad_model[:1] + bad_graph[:1] for b in short + [overflow, {"gram": None}]]
    pairs += [dict(no_model, **b) for b in [{}, {"beam_width": 129}, {"workspace_bytes": "short"}, {"state_bytes": "short"}]]
    out = []
    for m in singles + pairs:
        if all(k in base for k in m) and any(base[k] != v for k, v in m.items()) and m not in out:
            out.append(m)
    return out


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_covers_every_entry_and_never_launches():
    rows = _table()
    assert sorted({(r["entry"], r["variant"]) for r in rows}) == sorted((e, v) for e, vs in ENTRIES.items() for v in vs)
    for r in rows:
        assert r["code"] in (BAD_ARG, WORKSPACE, UNSUPPORTED), r          # never ASR_OK, never the launch code: nothing launches
        assert r["mutations"] in mutations_of(r["entry"], r["variant"]), r
    assert {r["code"] for r in rows} == {BAD_ARG, WORKSPACE, UNSUPPORTED}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_returns_the_recorded_codes(entry):
    from asr import _lib
    lib = _lib.lib()
    rows = [r for r in _table() if r["entry"] == entry]
    assert rows
    wrong = []
    for r in rows:
        got = run_case(lib, entry, r["variant"], r["mutations"])
        print(entry, r["variant"], json.dumps(r["mutations"], sort_keys=True), "->", got)
        if got != r["code"]:
            wrong.append((r["variant"], r["mutations"], "recorded %d" % r["code"], "got %d" % got))
    assert not wrong, wrong


def record():
    """writes the table from the library asr._lib loads (ASR_HIP_LIB): the mutations it answers with a code"""
    from asr import _lib
    assert not torch.cuda.is_available(), "record where there is no device: the valid calls would launch"
    lib = _lib.lib()
    rows = []
    for entry in sorted(ENTRIES):
        for variant in ENTRIES[entry]:
            assert run_case(lib, entry, variant, {}) == LAUNCH, (entry, variant)          # the starting point is a valid call
            for m in mutations_of(entry, variant):
                code = run_case(lib, entry, variant, m)
                if code in (BAD_ARG, WORKSPACE, UNSUPPORTED):
                    rows.append({"entry": entry, "variant": variant, "mutations": m, "code": code})
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print("%d rows from %s -> %s" % (len(rows), _lib.LIB_PATH, TABLE))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: ASR_HIP_LIB=<library to record from> python tests/test_beam_entry_codes_cpu.py --record")
    record()
