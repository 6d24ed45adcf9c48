"""The overlap table of tests/alias_cases.py against include/tcsfm.h, without a GPU: every ABI entry with an array parameter is either
a row of the table with all such parameters classified or an exemption with a reason -- so a new output added to the header fails here
until it is classified -- and the pairs the table honours are the ones the header's "overlapping arguments" section names."""
import os
import re

from conftest import REPO

import alias_cases as A


def _header():
    return open(os.path.join(REPO, "include", "tcsfm.h")).read()


def _prototypes():
    """{function: [(declaration, name) of every parameter]} of the header's tcsfm_* functions"""
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(tcsfm_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S):
        params = []
        for decl in m.group(2).split(","):
            decl = " ".join(decl.split())
            if decl in ("void", ""):
                continue
            name = re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?$", decl).group(1)
            params.append((decl, name))
        protos[m.group(1)] = params
    return protos


def _is_array(decl):
    return bool(re.search(r"\b(float|double)\s*\*", decl)) or "[" in decl


def test_the_parser_sees_the_whole_header():
    protos = _prototypes()
    from tightly_coupled_sfm_amd import _lib
    assert set(protos) == set(_lib.EXPORTS), set(protos) ^ set(_lib.EXPORTS)
    names = [n for _, n in protos["tcsfm_posenet_param_backward"]]
    assert names == ["pn", "N", "imgs", "tape", "d_pose", "d_imgs", "conv_w_g", "conv_b_g", "gn_w_g", "gn_b_g", "head_w_g", "head_b_g"]
    assert [n for d, n in protos["tcsfm_optim_step"] if _is_array(d)] == ["grads", "lr"]


def test_every_array_parameter_is_classified_or_exempt():
    protos = _prototypes()
    table = {r.entry for r in A.ROWS}
    assert not (table & set(A.EXEMPT)), table & set(A.EXEMPT)
    assert table <= set(protos) and set(A.EXEMPT) <= set(protos), (table | set(A.EXEMPT)) - set(protos)
    for fn, params in sorted(protos.items()):
        arrays = [n for d, n in params if _is_array(d)]
        if not arrays:
            assert fn not in table and fn not in A.EXEMPT, f"{fn} has no array parameter"
            continue
        if fn in A.EXEMPT:
            assert len(A.EXEMPT[fn]) > 10, fn
            continue
        assert fn in table, f"{fn}({', '.join(arrays)}) is neither a row of alias_cases.ROWS nor exempt"
        for r in A.rows_for(fn):
            assert [p.name for p in r.params] == arrays, (fn, [p.name for p in r.params], arrays)
            for p in r.params:
                assert p.role in (A.IN, A.OUT, A.HOST_OUT, A.HOST_IN), (fn, p.name)
                decl = next(d for d, n in params if n == p.name)
                # an output is not const-qualified at the element, an input is
                elem_const = bool(re.match(r"const\b", decl))
                assert elem_const == (p.role in (A.IN, A.HOST_IN)), (fn, decl, p.role)
    assert len(A.EXEMPT) <= 20


def test_rows_are_well_formed():
    ids = [A.row_id(r) for r in A.ROWS]
    assert len(set(ids)) == len(ids)
    for r in A.ROWS:
        names = [p.name for p in r.params]
        roles = {p.name: p.role for p in r.params}
        for o, i, kind in r.honoured:
            assert roles[o] == A.OUT and roles[i] == A.IN and kind in (A.SAME, A.ANY), (r.entry, o, i)
        if r.runner in ("generic", "sequence"):
            for p in r.params:
                assert p.shape is not None and (p.role != A.IN or p.gen is not None), (r.entry, p.name)
                if p.role == A.IN:
                    v = p.gen(p)
                    assert v.shape == tuple(p.shape) and v.dtype == p.dtype, (r.entry, p.name, v.shape, p.shape)
        assert len(names) == len(set(names)), r.entry


def test_honoured_pairs_are_the_headers():
    hdr = _header()
    sec = hdr[hdr.index("The honoured pairs, entry by entry"):hdr.index("(end of the honoured pairs")]
    named = {}
    for m in re.finditer(r"^ \*\s+(tcsfm_[a-z0-9_]+):\s*(.*)$", sec, flags=re.M):
        pairs = set()
        for item in m.group(2).split(","):
            o, kind, i = item.split()
            assert kind in (A.SAME, A.ANY), item
            pairs.add((o, i, kind))
        named[m.group(1)] = pairs
    table = {}
    for r in A.ROWS:
        if r.honoured:
            table.setdefault(r.entry, set()).update(r.honoured)
        for other in A.rows_for(r.entry):
            assert set(other.honoured) == set(r.honoured), r.entry
    assert named == table, {k: named.get(k, set()) ^ table.get(k, set()) for k in set(named) | set(table) if named.get(k) != table.get(k)}
    # the header's entries refer to the section
    assert hdr.count("overlapping arguments") >= 3
