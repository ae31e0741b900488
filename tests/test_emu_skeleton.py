"""The emulator restates the kernels' bodies by hand (tests/emu/wt_emu.cpp); this keeps the two from drifting: the ordered sequence of
wt_* phase calls and __syncthreads() of every kernel body, read off the HIP source as text, has to equal the sequence of the
emulator's driver for that kernel (its wt_* calls and barrier() / sub_barrier() marks) after the substitutions the emulator documents.
Adding or removing a barrier or a phase call on one side only turns this red, naming the kernel and the first interval that differs.
A text comparison: it does not understand `if constexpr`, only preprocessor conditionals with the default switches."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wiggletools_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu", "wt_emu.cpp")

# device-only call -> what the emulator runs in its place ("|": a loop boundary inside the substitute, sub_barrier() in the driver)
SUBST = {
    "wt_delta_ranges_w1": ["wt_delta_ranges1"],
    "wt_delta_ranges_w2": ["wt_delta_ranges2", "|", "wt_delta_ranges3"],
    "wt_walk_ranges_w2": ["wt_walk_ranges3"],
    "wt_delta_scan_w1": ["wt_delta_scan1", "|", "wt_delta_scan2"],
    "wt_delta_scan_w1_tt": ["wt_delta_scan1_tt", "|", "wt_delta_scan2_tt"],
    "wt_delta_scan_w1_mm": ["wt_delta_scan1_mm", "|", "wt_delta_scan2_mm"],
    "wt_delta_escan_wave": ["emu_escan_wave"],
}
EMU_NAMES = {"emu_walk_lanes": "wt_walk_lane", "emu_mwalk_lanes": "wt_mwalk_lane"}     # the stretch-walking rounds (real threads)
# not phases: set-up, the ticket counter, compile-time helpers, the profile builds' counters
IGNORE = {"wt_ctx_init", "wt_delta_ctx_init", "wt_walk_ctx_init", "wt_glb_add64", "wt_eval_passes", "wt_lds"}
DEFINED = {"WT_DELTA_ZERO_EARLY": 1}        # every other macro of an #if / #ifdef inside a kernel body is off (WT_PROFILE*, WT_MARK*)
KERNELS = [
    ("wt_reduce_kernel", "wt_reduce_kernel.h", "int NR = 0>\n    void run()"),       # (not WaveSched::run)
    ("wt_patch_kernel", "wt_patch_kernels.hip", "void run_patch()"),
    ("wt_delta_kernel", "wt_delta_kernel.h", "void run_delta()"),
    ("wt_walk_kernel", "wt_walk.hip", "void run_walk()"),
    ("wt_mwalk_kernel", "wt_walk.hip", "void run_mwalk()"),
]


def _strip_comments(s):
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


def _body(s, head):
    """the text between the braces of the function whose definition contains `head`"""
    i = s.index(head)
    i = s.index("{", s.index(")", i))
    depth, j = 0, i
    while True:
        if s[j] == "{":
            depth += 1
        elif s[j] == "}":
            depth -= 1
            if depth == 0:
                return s[i + 1:j]
        j += 1


def _preprocess(body):
    """#if / #ifdef / #ifndef / #elif / #else / #endif with DEFINED; #define lines (with continuations) dropped"""
    out, stack, lines, n = [], [], body.split("\n"), 0
    def cond(expr):
        expr = re.sub(r"defined\s*\(\s*(\w+)\s*\)", lambda m: "1" if m.group(1) in DEFINED else "0", expr)
        expr = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: str(DEFINED.get(m.group(0), 0)), expr)
        return bool(eval(expr.replace("!", " not ").replace("&&", " and ").replace("||", " or ")))
    while n < len(lines):
        line = lines[n]
        n += 1
        st = line.strip()
        if st.startswith("#"):
            d = st[1:].strip()
            if d.startswith("ifdef"):
                stack.append([d.split()[1] in DEFINED, False])
            elif d.startswith("ifndef"):
                stack.append([d.split()[1] not in DEFINED, False])
            elif d.startswith("if"):
                stack.append([cond(d[2:]), False])
            elif d.startswith("elif"):
                top = stack[-1]
                top[1] = top[1] or top[0]
                top[0] = (not top[1]) and cond(d[4:])
            elif d.startswith("else"):
                top = stack[-1]
                top[1] = top[1] or top[0]
                top[0] = not top[1]
            elif d.startswith("endif"):
                stack.pop()
            elif d.startswith("define"):
                while line.rstrip().endswith("\\"):
                    line = lines[n]
                    n += 1
            continue
        if all(t[0] for t in stack):
            out.append(line)
    return "\n".join(out)


def _drop_ep(body):
    """`if constexpr (EP) <block or statement> [else]`: Sum / Mean's early publish is wave code throughout; the emulator follows the
    kernel's other branch"""
    while True:
        m = re.search(r"if\s+constexpr\s*\(\s*EP\s*\)\s*", body)
        if not m:
            return body
        j = m.end()
        if body[j] == "{":
            depth = 0
            while True:
                depth += body[j] == "{"
                depth -= body[j] == "}"
                j += 1
                if depth == 0:
                    break
        else:
            j = body.index(";", j) + 1
        rest = re.match(r"\s*else\b", body[j:])
        body = body[:m.start()] + (body[j + rest.end():] if rest else body[j:])


TOKEN = re.compile(r"\b(__syncthreads|sub_barrier|barrier|(?:wt|emu)_[a-z0-9_]+)\s*(?:<[^;(){}]*?>)?\s*\(")


def _sequence(body, kernel_side):
    seq = []
    for m in TOKEN.finditer(body):
        name = m.group(1)
        if name in ("__syncthreads", "barrier"):
            seq.append("BARRIER")
        elif name == "sub_barrier":
            seq.append("|")
        elif name in IGNORE:
            continue
        elif kernel_side:
            seq.extend(SUBST.get(name, [name]))
        else:
            seq.append(EMU_NAMES.get(name, name))
    return seq


def _intervals(seq):
    out, cur = [], []
    for tok in seq:
        if tok == "BARRIER":
            out.append(cur)
            cur = []
        else:
            cur.append(tok)
    out.append(cur)
    return out


def kernel_sequence(name, src):
    s = _strip_comments(open(os.path.join(CSRC, src)).read())
    return _sequence(_drop_ep(_preprocess(_body(s, " %s(const WtParams" % name))), True)


def emulator_sequence(head):
    s = _strip_comments(open(EMU).read())
    return _sequence(_body(s, head), False)


def compare(name, kern, emu):
    a, b = _intervals(kern), _intervals(emu)
    for i in range(max(len(a), len(b))):
        x = a[i] if i < len(a) else None
        y = b[i] if i < len(b) else None
        if x != y:
            return "%s: interval %d of the kernel text is %s, of the emulator's driver %s" % (name, i + 1, x, y)
    return None


@pytest.mark.parametrize("name,src,head", KERNELS, ids=[k[0] for k in KERNELS])
def test_emulator_driver_has_the_kernels_phases_and_barriers(name, src, head):
    kern, emu = kernel_sequence(name, src), emulator_sequence(head)
    assert len(kern) > 15 and kern.count("BARRIER") >= 8, kern
    msg = compare(name, kern, emu)
    assert msg is None, msg


def test_a_removed_barrier_is_noticed():
    """the comparison itself: the delta kernel's text less one __syncthreads() (the one after wt_delta_load_res_tt) is red, and names it"""
    kern, emu = kernel_sequence("wt_delta_kernel", "wt_delta_kernel.h"), emulator_sequence("void run_delta()")
    i = kern.index("wt_delta_load_res_tt")
    assert kern[i + 1] == "BARRIER"
    msg = compare("wt_delta_kernel", kern[:i + 1] + kern[i + 2:], emu)
    assert msg is not None and "wt_delta_kernel: interval" in msg and "wt_delta_load_res_tt" in msg, msg
