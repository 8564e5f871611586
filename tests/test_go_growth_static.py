"""The Go plugin's side of the group-by table growth, checked on the source text (there is
no Go toolchain here): the new C functions resolve against include/gpuagg.h, growth is
turned on where the contexts are created, and publish counts what is still lost in
LostEventsCounter."""
import os
import re

from tests import go_static as gs


def _func_body(code: str, head: str) -> str:
    """The text of the top-level func whose declaration starts with `head`."""
    m = re.search(r"^func\s+" + head, code, re.M)
    assert m, head
    nxt = re.search(r"^func\b", code[m.end():], re.M)
    return code[m.start(): m.end() + nxt.start() if nxt else len(code)]


def _block(code: str, start: int) -> str:
    """The braced block that opens at or after `start`."""
    i = code.index("{", start)
    depth = 0
    for j in range(i, len(code)):
        depth += {"{": 1, "}": -1}.get(code[j], 0)
        if depth == 0:
            return code[i:j + 1]
    raise AssertionError("unbalanced block")


def _plugin():
    return gs.parse_go(os.path.join(gs.GO_PKG, "gpuagg_linux.go"))


def test_go_package_resolves_growth_functions():
    assert gs.all_errors() == []
    assert {"gpuagg_set_sparse_growth", "gpuagg_sparse_info", "GPUAGG_FLAG_REGROW_DIRECT"} <= gs.header_names()


def test_growth_is_set_where_contexts_are_created():
    code = _plugin().code
    creators = [m.group(1) for m in re.finditer(r"^func\s+(?:\([^)]*\)\s*)?(\w+)", code, re.M)
                if "C.gpuagg_create(" in _func_body(code, r"(?:\([^)]*\)\s*)?" + m.group(1) + r"\b")]
    assert creators, "no function calls gpuagg_create"
    for fn in creators:
        body = _func_body(code, r"(?:\([^)]*\)\s*)?" + fn + r"\b")
        assert body.index("C.gpuagg_set_sparse_growth(") > body.index("C.gpuagg_create("), fn
    assert re.search(r"\bsparseLog2\s*=\s*20\b", code) and re.search(r"\bsparseMaxLog2\s*=\s*26\b", code)


def test_publish_counts_lost_updates():
    body = _func_body(_plugin().code, r"\(g \*gpuAgg\) publish\b")
    m = re.search(r"if\s+lost\s*>\s*0", body)
    assert m, "publish has no lost-updates check"
    guarded = _block(body, m.end())
    assert "g.l.Warn(" in guarded  # the warning stays
    assert re.search(r"metrics\.LostEventsCounter\.WithLabelValues\(utils\.BufferedChannel,\s*name\)", guarded)
    assert "g.lostLast" in body  # the delta since the previous publish, not the cumulative count
