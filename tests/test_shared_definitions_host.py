"""CPU-only, sources only: the front end's shared definitions have ONE home each (docs/kernels.md 4.25).

(a) every function of the internal interface is declared in csrc/launch.hpp under the file that defines it, and defined there and
    nowhere else; the split contraction's primitives are defined in csrc/split_f16.hpp only, the solvers' guard, uni() and
    align256() in csrc/common.hpp only, mul_rcp() / load9() in csrc/lane_reduce.hpp only - and the spellings they replaced are gone;
(b) no .hip / .cpp under csrc/ declares, at namespace scope, a function it does not define (a declaration: a statement ending in
    `);` that is not static, extern "C", a template or a definition) - an interface is declared in a header its definition sees."""
import os
import re

from conftest import REPO

CSRC = os.path.join(REPO, "pats_amd", "csrc")


def sources():
    out = {}
    for root, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".hip", ".cpp", ".hpp")):
                out[os.path.relpath(os.path.join(root, f), CSRC)] = open(os.path.join(root, f)).read()
    return out


def strip(text):
    """comments, string contents and preprocessor lines out; line numbers stay"""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)


def statements(text):
    """[(line, head, has_body)] of the namespace-scope statements: `namespace ... {` and `extern "C" {` are looked into, every
    other brace pair is a body and skipped; head = the text up to the `;` or up to the body"""
    out, i, start, par = [], 0, 0, 0
    while i < len(text):
        c = text[i]
        par += (c == "(") - (c == ")")
        if par == 0 and c == ";":
            out.append((text.count("\n", 0, start) + 1, " ".join(text[start:i + 1].split()), False))
            start = i + 1
        elif par == 0 and c == "{":
            head = " ".join(text[start:i].split())
            if re.match(r'^(namespace( \w+)?|extern "")$', head):
                start = i + 1
            else:
                depth, j = 1, i + 1
                while depth and j < len(text):
                    depth += (text[j] == "{") - (text[j] == "}")
                    j += 1
                out.append((text.count("\n", 0, start) + 1, head, True))
                m = re.match(r"\s*;", text[j:])            # struct X { ... };
                i = j + (m.end() if m else 0) - 1
                start = i + 1
        elif par == 0 and c == "}":
            start = i + 1
        i += 1
    return out


def function_name(head):
    m = re.search(r"([A-Za-z_]\w*)\s*(?:<[^()]*>)?\s*\(", head)
    return m.group(1) if m else None


def defined_functions(text):
    return {function_name(h) for _, h, body in statements(strip(text)) if body}


def homes(pattern, src):
    return sorted(f for f, text in src.items() if re.search(pattern, strip(text)))


def test_every_shared_definition_has_one_home():
    src = sources()
    defined = {f: defined_functions(text) for f, text in src.items()}
    # launch.hpp: `// <file>` opens a group, every declaration below it is of a function that file - and no other - defines
    home, declared = None, {}
    for line in src["launch.hpp"].split("namespace pats {")[1].splitlines():
        m = re.match(r"^// (\w+\.(?:hip|cpp))\b", line)
        if m:
            home = m.group(1)
        m = re.match(r"^(?:template <typename T> )?[\w:]+[ *&]+(?:\w+[ *&]+)*?(\w+)\(", line)
        if m and not line.startswith("//"):
            assert m.group(1) not in declared, "declared twice in launch.hpp: " + m.group(1)
            declared[m.group(1)] = home
    assert len(declared) >= 38 and "launch_cost65" in declared and "launch_fine_out" in declared, sorted(declared)
    for name, f in declared.items():
        assert [g for g in defined if name in defined[g]] == [f], (name, f)
        assert '#include "launch.hpp"' in src[f], f + " defines " + name + " without seeing its declaration"
    for name in ("launch_third_fused", "launch_third_fused3"):
        assert homes(r"\bint %s\([^;{}]*\);" % name, src) == ["third_device.hpp"], name     # the declaration
    # the homes of items 2 and 3: a definition = a function with a body, a typedef, or a constexpr constant
    for f, functions, typedefs, constants in (
            ("split_f16.hpp", ("split4", "split4_pre", "split8", "mfma3", "uniform_ptr", "fma4", "bcast4"),
             ("h8v", "h4v", "h2v", "f4v", "f2v", "gptr_h8"), ("PRE", "UNS")),
            ("common.hpp", ("scaling_ok", "uni", "align256"), (), ("SCALE_GUARD",)),
            ("lane_reduce.hpp", ("mul_rcp", "load9"), (), ())):
        for name in functions:
            assert [g for g in defined if name in defined[g]] == [f], name
        for name in typedefs:
            assert homes(r"\btypedef\b[^;]*[ *]%s(;| __attribute__)" % name, src) == [f], name
        for name in constants:
            assert homes(r"\bconstexpr float\b[^;]*\b%s =" % name, src) == [f], name
    for gone in (r"\bPRESCALE\b", r"\bUNSCALE\b", r"\bC65_PRESCALE\b", r"\bBLK_GUARD\b", r"\bW2_GUARD\b", r"\bGUARD =", r"\bok_scale\b",
                 r"\bsc_ok\b", r"\bal256\("):
        assert homes(gone, src) == [], gone
    assert homes(r"1073741824", src) == ["common.hpp"]                      # the guard as a bare literal
    assert "split_model" in src["split_f16.hpp"] and "docs/parity.md" in src["split_f16.hpp"]          # the model that tests the contract


def test_no_source_file_declares_a_function_it_does_not_define():
    found = []
    for f, text in sources().items():
        if f.endswith(".hpp"):
            continue
        st = statements(strip(text))
        own = {function_name(h) for _, h, body in st if body}
        for line, h, body in st:
            if body or not h.endswith(");") or re.match(r'^(static\b|static_assert|extern ""|template\b|typedef\b|using\b)', h):
                continue
            if "=" in h.split("(")[0]:                                      # a variable initialised by a call
                continue
            if function_name(h) not in own:
                found.append("%s:%d %s" % (f, line, h[:100]))
    assert not found, "\n".join(found)
