"""CPU side of the loop-closure residual report and the chi-square gated solve: the C-ABI surface in capi.py, the layout of
dsss_pg_gate_params against the header text, and the gate rule run on the oracle alone on the four corrupted lawnmower graphs
(the fixture tests/test_gpu_pg_report.py holds the device to)."""
import ctypes as C
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CTYPES = {"double": C.c_double, "int32_t": C.c_int32, "int": C.c_int, "float": C.c_float, "uint8_t": C.c_uint8, "int64_t": C.c_int64}


def _header_struct(name):
    """[(field, C type name)] of `typedef struct { ... } name;` in include/dsss.h"""
    hdr = open(os.path.join(ROOT, "include", "dsss.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % re.escape(name), hdr)
    assert m, name
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = decl.split(None, 1)
        fields += [(n.strip(), ty) for n in names.split(",")]
    return fields


def test_gate_params_match_the_header():
    from diasss_amd import capi
    fields = _header_struct("dsss_pg_gate_params")
    assert [f for f, _ in fields] == ["gate", "decade", "max_solves", "pad_"]
    off, align = 0, 1
    for (name, ty), (pname, pty) in zip(fields, capi.PGGateParams._fields_):
        ct = _CTYPES[ty]
        a = C.alignment(ct); align = max(align, a)
        off = (off + a - 1) // a * a                                  # natural alignment, as the C compiler lays the struct out
        d = getattr(capi.PGGateParams, name)
        assert pname == name and pty is ct and d.offset == off and d.size == C.sizeof(ct), name
        off += C.sizeof(ct)
    assert C.sizeof(capi.PGGateParams) == (off + align - 1) // align * align == 24


def test_capi_declares_the_report_and_the_gated_solve():
    from diasss_amd import capi
    L = capi.lib()
    rep, gat, dflt = L.dsss_posegraph_edge_report, L.dsss_posegraph_solve_gated, L.dsss_pg_gate_params_default
    assert rep.restype is C.c_int and len(rep.argtypes) == 9 and rep.argtypes[2] is C.c_int and rep.argtypes[4] is C.c_int
    assert gat.restype is C.c_int and len(gat.argtypes) == 11 and gat.argtypes[5] is C.POINTER(capi.PGGateParams) and gat.argtypes[10] is C.POINTER(C.c_int)
    g = capi.PGGateParams(); dflt(C.byref(g))
    assert (g.gate, g.decade, g.max_solves) == (22.458, 10.0, 8)
    for name in ("posegraph_edge_report", "posegraph_solve_gated", "gate_params_default"):
        assert callable(getattr(capi.Context, name))


@pytest.mark.parametrize("case", range(4))
def test_gate_rule_on_the_oracle(orc, case):
    """the rule on the oracle alone: solves, corrupted edges kept (none), clean edges dropped, and no kept edge within 1 % of a
    round's threshold -- so a 1e-6 difference in the poses cannot flip a decision of the device's run of the same rule"""
    from tests import pg_report_ref as R
    args, frac, solves, nbad, ndrop, nclean = R.GATE_GRAPHS[case]
    dr, edges, bad = R.corrupted_graph(args, frac)
    assert bad.sum() == nbad and (~bad).sum() == nclean
    poses, keep, ns, margin = R.oracle_gate(orc, dr, edges)
    print("graph %s frac %.2f: %d solves, corrupted kept %d of %d, clean dropped %d of %d, closest margin %.1f %%"
          % (args, frac, ns, (keep & bad).sum(), nbad, (~keep & ~bad).sum(), nclean, 100 * margin))
    assert ns == solves
    assert not (keep & bad).any()
    assert (~keep & ~bad).sum() == ndrop and ndrop <= 0.05 * nclean
    assert margin > 0.01
    # the kept edges agree with the returned trajectory: the rule stopped because of the gate, not because it ran out of solves
    xi, sg = R.edge_residuals(orc, edges[keep], poses)
    assert ((xi / sg) ** 2).sum(axis=1).max() <= R.GATE and ns < R.MAX_SOLVES
