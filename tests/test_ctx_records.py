"""Every device buffer, pinned mirror and cloud a record of csrc/rgc_ctx.h declares is listed in its bufs() / pinned() / clouds(), and rgc_destroy
releases every record of struct rgc_ctx (no GPU: the header and rgc_api.hip are parsed).

A buffer that is declared and then forgotten in bufs() leaks silently; a large one shows in tests/test_gpu_*_release.py, a 16-byte one only here.

What is read as what, the header's own conventions:
  * a record is a struct with a bufs(); its members are what stands at the struct's own brace depth (nested types' and functions' bodies are not members),
    and its base's (`struct X : Base {`): NoLists brings empty pinned() / clouds(), FrameLists an OpFrame f with its two lists;
  * `DevBuf a, b[4];` declares device buffers: `&a` must appear in bufs(), and of an array every `&b[i]`, or a loop `for (DevBuf& x : b)`;
  * every non-const raw pointer member of a record is a pinned mirror and must appear in pinned() (none is exempt today: NOT_PINNED); so must `m.p` of
    a `PinnedBuf m`;
  * `Cloud c, d[2];` declares clouds: `&c`, `&d[0]`, `&d[1]` must appear in clouds();
  * a member whose type is a struct at namespace scope (Sums, Selection, OpFrame, PinnedBuf) counts through the member's name: `Sums sums;` brings
    `&sums.partials`, `&sums.out` and `sums.h_out`;
  * a member of struct rgc_ctx whose type is a record needs a `release_record(c-><member>)` in rgc_api.hip."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgc-slam_amd", "csrc")


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def _strip_comments(s):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def _close(s, i):
    """the index of the brace that closes the one at s[i]"""
    d = 0
    for j in range(i, len(s)):
        d += s[j] == "{"
        d -= s[j] == "}"
        if d == 0:
            return j
    raise ValueError("unbalanced braces")


NOT_PINNED = set()      # "Record::member" of raw pointers that are no pinned mirrors, should a record ever hold one


def _structs(s):
    """{name: body} of every struct defined in s, nested ones included under their own name; a base's body stands behind the struct's own"""
    out = {}
    for m in re.finditer(r"\bstruct\s+(\w+)\s*(?::\s*(\w+)\s*)?\{", s):
        out[m.group(1)] = s[m.end():_close(s, m.end() - 1)] + out.get(m.group(2), "")
    return out


def _raw_pointers(own):
    """the non-const raw pointer members among the declarations"""
    out = []
    for stmt in own.split(";"):
        m = re.fullmatch(r"\s*((?:[\w:]+\s+)*[\w:]+)\s*\*\s*(\w+)\s*(?:=[^()]*)?", stmt)
        if m and "(" not in stmt and not re.search(r"\bconst\b", m.group(1)):
            out.append((m.group(2), None))
    return out


def _own_level(body):
    """body without what stands inside braces: the declarations of the struct itself"""
    out, d = [], 0
    for ch in body:
        if ch == "{":
            d += 1
        elif ch == "}":
            d -= 1
            out.append(" ")     # `struct X { ... } name;` and `f() { ... }` both leave a separator
        elif d == 0:
            out.append(ch)
    return "".join(out)


def _method(body, name):
    m = re.search(r"\b" + name + r"\(\)\s*\{", body)
    return None if not m else body[m.end():_close(body, m.end() - 1)]


def _declared(own, type_name, pointer=False):
    """[(name, array size or None)] of the members of that type"""
    out = []
    pat = r"(?<![\w:<])" + type_name + (r"\s*\*\s*" if pointer else r"\s+") + r"(?![*&])([^;()]*);"
    for m in re.finditer(pat, own):
        for item in m.group(1).split(","):
            item = item.split("=")[0].strip().lstrip("*").strip()
            a = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", item)
            if a:
                out.append((a.group(1), a.group(2)))
    return out


def _members(structs, name, consts):
    """(device buffers, pinned pointers, clouds) of struct `name` as the expressions its lists must hold; arrays as (name, n or None)"""
    own = _own_level(structs[name])
    bufs = _declared(own, "DevBuf")
    clouds = _declared(own, "Cloud")
    pinned = [(n, k) for n, k in _raw_pointers(own) if name + "::" + n not in NOT_PINNED]
    for inner in ("Sums", "Selection", "OpFrame", "PinnedBuf"):
        if inner == name or inner not in structs:
            continue
        for m, k in _declared(own, inner):
            assert k is None, "an array of %s in %s: not a shape this check knows" % (inner, name)
            b, p, c = _members(structs, inner, consts)
            bufs += [(m + "." + n, kk) for n, kk in b]
            pinned += [(m + "." + n, kk) for n, kk in p]
            clouds += [(m + "." + n, kk) for n, kk in c]
    return bufs, pinned, clouds


def _listed(body, name, size, consts, address):
    """is member `name` (an array of `size` when not None) in the list function's body?"""
    amp = r"&\s*" if address else r"(?<![\w.&])"
    if size is None:
        return re.search(amp + re.escape(name) + r"(?![\w\[.])", body) is not None
    if re.search(r"for\s*\([^)]*:\s*" + re.escape(name) + r"\s*\)", body):
        return True
    n = int(size) if size.isdigit() else consts.get(size)
    return n is not None and all(re.search(amp + re.escape(name) + r"\[" + str(i) + r"\]", body) for i in range(n))


def problems(ctx_h, api_hip, public_h):
    """what is declared and not listed, as a list of sentences (empty: all is well)"""
    s = _strip_comments(ctx_h)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"(?:#define\s+|\b)(RGC_\w+)\s*=?\s*(\d+)\b", _strip_comments(public_h))}   # macros, enumerators
    structs = _structs(s)
    records = [n for n, b in structs.items() if _method(b, "bufs") is not None]
    out = []
    for r in records:
        bufs, pinned, clouds = _members(structs, r, consts)
        for what, members, address in (("bufs", bufs, True), ("pinned", pinned, False), ("clouds", clouds, True)):
            body = _method(structs[r], what)
            if body is None:
                out.append("%s has no %s()" % (r, what))
                continue
            for name, size in members:
                if not _listed(body, name, size, consts, address):
                    out.append("%s::%s is not in %s::%s()" % (r, name + ("[%s]" % size if size else ""), r, what))
    api = _strip_comments(api_hip)
    for m in re.finditer(r"(?:rgcapi::)?(\w+)\s+(\w+)\s*;", _own_level(structs["rgc_ctx"])):
        if m.group(1) in records and not re.search(r"release_record\(c->" + m.group(2) + r"\)", api):
            out.append("rgc_destroy has no release_record(c->%s)" % m.group(2))
    return records, out


def _sources():
    return _read(CSRC, "rgc_ctx.h"), _read(CSRC, "rgc_api.hip"), _read(ROOT, "include", "rgc_hip.h")


def test_every_buffer_mirror_and_cloud_of_a_record_is_listed_and_every_record_released():
    records, bad = problems(*_sources())
    print(len(records), "records:", " ".join(records))
    for name in ("Sums", "NdtRecord", "GicpRecord", "GicpStRecord", "GicpMpRecord", "SearchRecord", "OutlierRecord", "ClusterRecord", "PlaneRecord", "NormalRecord",
                 "FpfhRecord", "MapregRecord", "RollingMapRecord", "KeyframeRecord", "PgoRecord", "LeafFilterRecord", "FrontendRecord"):
        assert name in records, name
    assert bad == [], "\n".join(bad)


def test_the_check_sees_a_forgotten_member():
    """the same parse on copies of the header with one name dropped from a list, and of rgc_api.hip with one release dropped"""
    h, api, pub = _sources()
    for drop, said in ((("&partials, &small};", "&partials};"), "MapregRecord::small is not in MapregRecord::bufs()"),
                       (("&store[2], &table", "&table"), "KeyframeRecord::store[RGC_KF_KINDS] is not in KeyframeRecord::bufs()"),
                       (("&partials, &sel.flag, &sel.off, &sel.bs, &sel.out, &sel.idx}", "&partials, &sel.flag, &sel.off, &sel.bs, &sel.out}"),
                        "OutlierRecord::sel.idx is not in OutlierRecord::bufs()"),
                       (("return {h_table.p};", "return {};"), "KeyframeRecord::h_table.p is not in KeyframeRecord::pinned()"),
                       (("return {sums.h_out, h_small};", "return {sums.h_out};"), "NdtRecord::h_small is not in NdtRecord::pinned()"),
                       (("return {&aux};", "return {};"), "LeafFilterRecord::aux is not in LeafFilterRecord::clouds()"),
                       (("for (DevBuf& b : buf) v.push_back(&b);", ""), "FrontendRecord::buf[kFeBufs] is not in FrontendRecord::bufs()")):
        assert h.count(drop[0]) == 1, drop[0]
        assert problems(h.replace(*drop), api, pub)[1] == [said], drop
    assert api.count("  release_record(c->pgo);\n") == 1
    assert problems(h, api.replace("  release_record(c->pgo);\n", ""), pub)[1] == ["rgc_destroy has no release_record(c->pgo)"]
