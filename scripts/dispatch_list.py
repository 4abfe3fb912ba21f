"""The kernel dispatches of one run, in dispatch order, as `kernel name, grid, workgroup size`: from the kernel-trace CSV that
`rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- PROGRAM` leaves under DIR.  Two runs that queue the same work print the same
list whatever the kernels' timing was (profiles/driver_stages_dispatches_*.txt).

A kernel name longer than 120 characters is cut there and followed by a hash of the whole name.  The list is folded without loss:
`N x line` stands for N consecutive dispatches of that line, and `repeat N {` ... `}` for N consecutive copies of the lines between
(a loop of the driver; the blocks do not nest).

usage: python3 scripts/dispatch_list.py DIR_OR_CSV [section title]"""
import csv
import glob
import hashlib
import os
import sys

MAX_PERIOD = 400
MAX_NAME = 120


def short_name(name):
    """library kernels (rocprim) have names of thousands of characters: the first MAX_NAME and a hash of the whole"""
    return name if len(name) <= MAX_NAME else f"{name[:MAX_NAME]}...#{hashlib.sha1(name.encode()).hexdigest()[:12]}"


def dispatches(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if len(found) != 1:
            sys.exit(f"{path}: expected one *kernel_trace.csv, found {len(found)}")
        path = found[0]
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        yield f'{short_name(r["Kernel_Name"])}, {grid}, {wg}'


def runs(lines):
    """consecutive equal lines -> [line, count]"""
    out = []
    for ln in lines:
        if out and out[-1][0] == ln:
            out[-1][1] += 1
        else:
            out.append([ln, 1])
    return out


def compact(lines):
    """The list with runs of one line and repeated blocks folded; expand() gives the list back."""
    items = [f"{n} x {ln}" if n > 1 else ln for ln, n in runs(lines)]
    out, i = [], 0
    while i < len(items):
        best_p, best_k = 0, 1
        for p in range(2, min(MAX_PERIOD, (len(items) - i) // 2) + 1):
            k = 1
            while items[i + k * p:i + (k + 1) * p] == items[i:i + p]:
                k += 1
            if k > 1 and (k - 1) * p > (best_k - 1) * best_p:
                best_p, best_k = p, k
        if best_k > 1:
            out += [f"repeat {best_k} {{"] + ["  " + x for x in items[i:i + best_p]] + ["}"]
            i += best_p * best_k
        else:
            out.append(items[i])
            i += 1
    return out


def expand(text_lines):
    out, block, times = [], None, 0
    for ln in text_lines:
        if ln.startswith("repeat ") and ln.endswith(" {"):
            block, times = [], int(ln.split()[1])
            continue
        if ln == "}":
            out += block * times
            block = None
            continue
        ln = ln[2:] if block is not None else ln
        head, sep, rest = ln.partition(" x ")
        one = [rest] * int(head) if sep and head.isdigit() else [ln]
        (block if block is not None else out).extend(one)
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    lines = list(dispatches(sys.argv[1]))
    short = compact(lines)
    assert expand(short) == lines
    if len(sys.argv) > 2:
        print(f"## {sys.argv[2]} ({len(lines)} dispatches)")
    print("\n".join(short))
