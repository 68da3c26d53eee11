"""Every blocking or null-stream HIP call of the native sources is written down, with the reason it is safe.

The ABI's first convention (include/esmdiff_hip.h) is that all work goes to the caller's stream and nothing waits unless the
header says so.  A call that breaks it is easy to add and invisible on the null stream, so this test lists them from the source
text — every blocking hipMemcpy* / hipMemset* (hipMemcpy(, hipMemset(, hipMemcpyFromSymbol(, ... : the names without Async),
hipDeviceSynchronize, any kernel launch or *Async call whose stream argument is 0 / nullptr, and any call of one of the project's own
launch_* launchers whose last argument is 0 / nullptr (the launchers take the stream last or near last; where the last argument
is something else, the row's reason says so) — and compares the list (file, function, call, how many) with tests/stream_calls_allowed.json.  A new one fails here until someone
has added it to the list with a one-line reason; one that went away must leave the list too.
"""
import json
import re
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "esmdiff_amd" / "csrc"
ALLOWED = Path(__file__).resolve().parent / "stream_calls_allowed.json"

BLOCKING = re.compile(r"^(hipDeviceSynchronize|hip(Memcpy|Memset)(?!\w*Async)\w*)$")
NOT_A_FUNCTION = {"if", "for", "while", "switch", "catch", "return", "sizeof", "defined"}


def strip_comments_and_strings(text: str) -> str:
    """The source with comments and the contents of string / character literals blanked out, newlines kept."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            # a comment line may end in a backslash inside a macro: keep the continuation
            out.append(" " * (j - i - 1) + ("\\" if text[j - 1] == "\\" else " "))
            i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j]))
            i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c)
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def call_args(text: str, open_paren: int):
    """The top-level arguments of the call whose '(' is at open_paren, and the index after its ')'."""
    depth, args, start, i = 0, [], open_paren + 1, open_paren
    while i < len(text):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                last = text[start:i].strip()
                if last or args:
                    args.append(last)
                return args, i + 1
        elif c == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
        i += 1
    raise ValueError("unbalanced call")


def functions(text: str):
    """[(start, end, name)]: the bodies of the function definitions (outermost only) and of the #define macros."""
    spans = []
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(?:[^\n]*\\\n)*[^\n]*", text, re.M):
        spans.append((m.start(), m.end(), "#define " + m.group(1)))
    in_macro = lambda p: any(s <= p < e for s, e, _ in spans)
    depth, cur, seg = 0, None, 0        # cur = (name, depth at its '{', start)
    for i, c in enumerate(text):
        if in_macro(i):
            continue
        if c == "{":
            if cur is None:
                head = re.sub(r"^[ \t]*#[^\n]*$", " ", text[seg:i], flags=re.M)   # (preprocessor lines between definitions)
                m = re.search(r"([A-Za-z_]\w*)\s*\((?:[^()]|\([^()]*\))*\)\s*(?:const\s*)?$", head)
                if m and m.group(1) not in NOT_A_FUNCTION:
                    cur = (m.group(1), depth, i)
            depth += 1
            seg = i + 1
        elif c == "}":
            depth -= 1
            if cur is not None and depth == cur[1]:
                spans.append((cur[2], i + 1, cur[0]))
                cur = None
            seg = i + 1
        elif c == ";" and cur is None:
            seg = i + 1
    return spans


def is_null_stream(arg: str) -> bool:
    a = re.sub(r"\s+", "", arg)
    a = re.sub(r"^\(?\(hipStream_t\)(.*?)\)?$", r"\1", a)
    return a in ("0", "nullptr", "NULL", "hipStreamDefault")


def scan_text(text: str):
    """[(function, call)] for every blocking or null-stream HIP call in one source text."""
    clean = strip_comments_and_strings(text)
    spans = functions(clean)

    def where(p):
        inner = [s for s in spans if s[0] <= p < s[1]]
        return min(inner, key=lambda s: s[1] - s[0])[2] if inner else "<file scope>"

    found = []
    for m in re.finditer(r"\b((?:hip|launch_)\w+)\s*(\()?", clean):
        name, p = m.group(1), m.start()
        if name.startswith("launch_"):
            # a call, not the launcher's own definition or declaration (those have typed parameters, never a bare 0 / nullptr)
            if m.group(2):
                args, _ = call_args(clean, m.end() - 1)
                if args and is_null_stream(args[-1]):
                    found.append((where(p), "%s(last argument %s)" % (name, re.sub(r"\s+", "", args[-1]))))
        elif BLOCKING.match(name) and (m.group(2) or name == "hipDeviceSynchronize"):
            found.append((where(p), name))
        elif m.group(2) and (name == "hipLaunchKernelGGL" or name.endswith("Async")):
            args, _ = call_args(clean, m.end() - 1)
            if name == "hipLaunchKernelGGL":
                stream = args[4] if len(args) > 4 else "0"
            else:
                stream = args[-1] if args else "0"
            if is_null_stream(stream):
                found.append((where(p), "%s(stream %s)" % (name, re.sub(r"\s+", "", stream))))
    for m in re.finditer(r"<<<", clean):     # a triple-chevron launch names its stream fourth; fewer means the null stream
        j = clean.find(">>>", m.end())
        args, _ = call_args("(" + clean[m.end():j] + ")", 0)
        if len(args) < 4 or is_null_stream(args[3]):
            found.append((where(m.start()), "<<<launch on the null stream>>>"))
    return found


def scan_tree():
    rows = Counter()
    for f in sorted(CSRC.iterdir()):
        if f.suffix in (".hip", ".h", ".inc"):
            for fn, call in scan_text(f.read_text()):
                rows[(f.name, fn, call)] += 1
    return rows


def test_the_scanner_sees_what_it_should():
    src = '''
    // hipMemcpy(a, b, 4, k) in a comment does not count
    namespace {
    int helper(int a) { const char* s = "hipDeviceSynchronize()"; return a; }
    }
    #define LAUNCH(N) hipLaunchKernelGGL((kern<N>), grid, block, 0, stream, x) \\
      ; hipMemsetAsync(p, 0, 4, 0)
    extern "C" {
    int entry(void* stream) {
      hipStream_t st = (hipStream_t)stream;
      if (x) { hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice); }
      hipMemcpyAsync(dst, src, f(n, 2), hipMemcpyDeviceToDevice, st);
      hipMemcpyAsync(dst, src, f(n, 2), hipMemcpyDeviceToDevice, nullptr);
      hipLaunchKernelGGL(k2, dim3(1), dim3(64), 0, 0, x);
      hipLaunchKernelGGL((k3<1, 2>), dim3(g(1, 2)), dim3(64), 0, st, x);
      auto f = [&](int v) { return hipDeviceSynchronize(); };
      k4<<<1, 64>>>(x);
      k4<<<1, 64, 0, st>>>(x);
      hipMemcpyFromSymbol(&h, sym, 4);
      hipMemsetAsync(p, 0, 4, st);
      launch_thing(a, b, st);
      launch_thing(a, f(b, 0), 0);
      return 0;
    }
    }
    '''
    assert sorted(scan_text(src)) == sorted([
        ("#define LAUNCH", "hipMemsetAsync(stream 0)"),
        ("entry", "hipMemcpy"),
        ("entry", "hipMemcpyAsync(stream nullptr)"),
        ("entry", "hipLaunchKernelGGL(stream 0)"),
        ("entry", "hipDeviceSynchronize"),
        ("entry", "<<<launch on the null stream>>>"),
        ("entry", "hipMemcpyFromSymbol"),
        ("entry", "launch_thing(last argument 0)"),
    ])


def test_every_blocking_or_null_stream_call_is_on_the_allow_list():
    allowed = json.loads(ALLOWED.read_text())
    want = Counter()
    for row in allowed:
        key = (row["file"], row["function"], row["call"])
        assert key not in want, f"listed twice: {key}"
        assert len(row["reason"].strip()) >= 12 and "\n" not in row["reason"], f"{key}: give a one-line reason"
        want[key] = int(row["count"])
    found = scan_tree()
    new = {k: (n, want.get(k, 0)) for k, n in found.items() if n > want.get(k, 0)}
    gone = {k: (found.get(k, 0), n) for k, n in want.items() if n > found.get(k, 0)}
    assert not new, ("blocking or null-stream HIP calls that tests/stream_calls_allowed.json does not allow (found, allowed): "
                     "write down why each is safe on a caller's non-blocking stream, or put it on the caller's stream\n" +
                     "\n".join(f"  {k}: {v}" for k, v in sorted(new.items())))
    assert not gone, ("tests/stream_calls_allowed.json allows calls the sources no longer make (found, allowed): remove them\n" +
                      "\n".join(f"  {k}: {v}" for k, v in sorted(gone.items())))
    assert sum(found.values()) > 30      # the scan found the tree
