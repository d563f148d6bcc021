"""GPU tests move arrays between host and device only through
tests/gpu_copies.py (pinned buffers).  Every test file
that carries the ``gpu`` mark is read as text: a line with a pageable copy
idiom fails unless it ends with ``# pageable: <reason>``, and at most 8 lines
of the whole suite may.  (``.tolist()`` of a device tensor reads like numpy's
and is left to review.)"""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ONE_LINE = re.compile(r"\.cpu\(|\.cuda\(|\.item\(")
# the two halves of these may stand on different lines of one statement
SPLIT = re.compile(r"from_numpy\(.*\.to\(|torch\.(as_)?tensor\(.*\bdevice\s*=", re.S)
SPLIT_HEAD = re.compile(r"from_numpy\(|torch\.(as_)?tensor\(")
KEPT = re.compile(r"# pageable: \S")
MAX_KEPT = 8
REACH = 3  # lines of a statement looked at after the one that opens it


def _statement(lines, i):
    """lines[i] with the lines its open brackets run on to, REACH at the most"""
    depth, text = 0, ""
    for line in lines[i:i + 1 + REACH]:
        text += line
        code = line.split("#", 1)[0]
        depth += sum(map(code.count, "([{")) - sum(map(code.count, ")]}"))
        if depth <= 0:
            break
    return text


def test_gpu_tests_copy_through_the_pinned_helpers():
    bad, kept = [], []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        lines = open(path).readlines()
        if os.path.samefile(path, __file__) or "mark.gpu" not in "".join(lines):
            continue
        for i, line in enumerate(lines):
            where = f"{os.path.basename(path)}:{i + 1}"
            if KEPT.search(line):
                kept.append(where)
            elif ONE_LINE.search(line) or (SPLIT_HEAD.search(line) and SPLIT.search(_statement(lines, i))):
                bad.append(f"{where}: {line.strip()}")
    assert not bad, f"{len(bad)} pageable host/device copies in GPU test files:\n" + "\n".join(bad)
    assert len(kept) <= MAX_KEPT, f"more than {MAX_KEPT} lines kept pageable: {kept}"
