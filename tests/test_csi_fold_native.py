"""The generalised index fold and its serialisers (svtyper_amd/csrc/svt_tbx_index.h, svt_bai_index.h, svt_index_scheme.h) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_csi_fold_main.cpp (its own main, the
headers compiled into it with -fsanitize=address,undefined).  The BAM inputs of tests/baicases.py and tests/csioutcases.py as span
tables and the texts of tests/tbxcases.py, each folded as CSI and compared with the plain-Python restatement, then folded as
CSI and as .bai / .tbi over the table truncated at every length -- each table in a heap buffer of exactly its length.  Host code
only; nothing is preloaded and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import baicases as B
import csioutcases as K
import tbxcases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
SHARES = 4      # runs of the program at the same time


class Laid:
    """a case's records in sorted order behind its header, in members cut as the writer cuts them at made-up file offsets: what
    csioutcases.build_csi_bam asks of a baicases.Written"""

    def __init__(self, case):
        self.header, self.n_ref = case.header, case.n_ref
        self.records = [case.records[i] for i in B.order(case.records, case.n_ref)]
        self.rows = [B.span(raw, case.n_ref) for raw in self.records]
        self.offsets, at = [], len(case.header)
        for raw in self.records:
            self.offsets.append(at)
            at += len(raw)
        self.starts = [0]
        for p in B.payloads(case.header, self.records):
            self.starts.append(self.starts[-1] + len(p))
        self.member_off = [0]
        for k in range(len(self.starts) - 1):
            self.member_off.append(self.member_off[-1] + 26 + (self.starts[k + 1] - self.starts[k]) // 3)

    def voffset(self, pos):
        for k in range(len(self.starts) - 2, -1, -1):
            if self.starts[k] <= pos < self.starts[k + 1]:
                return self.member_off[k] << 16 | (pos - self.starts[k])
        return self.member_off[-1] << 16


def bam_row(case):
    w = Laid(case)
    table = "".join("%d,%d,%d,%d,%d,%d,%d;" % ((at, len(raw)) + (row[0], row[1] & 0xFFFFFFFFFFFFFFFF, row[2], row[3], row[4]))
                    for at, raw, row in zip(w.offsets, w.records, w.rows)) or "-"
    refuse = getattr(case, "refuse", None)
    if refuse is not None and len(refuse) == 2:                 # (csioutcases: the record's number in the caller's order)
        want = "!%d,%d" % (w.records.index(case.records[refuse[0] - 1]) + 1, refuse[1])
    else:
        want = K.build_csi_bam(w).hex()
    return "B %d %d %s %s %s %s" % (case.n_ref, K.l_ref_max(case.header), table, ",".join(map(str, w.starts)), ",".join(map(str, w.member_off)), want), len(w.records)


def vcf_row(text, payload=X.PAYLOAD):
    n_members = (len(text) + payload - 1) // payload
    member_off = [1000 * k for k in range(n_members + 1)]
    return "V %d %s %s %s" % (payload, text.hex() or "-", ",".join(map(str, member_off)), K.build_csi_vcf(text, member_off, payload).hex()), len(X.split_lines(text))


def cases_text():
    rows = [bam_row(case) for _label, case in K.all_indexable()] + [bam_row(K.CASES[name]) for name in K.REFUSED]
    texts = dict(X.TEXTS)
    texts["beyond_2_29"] = X.HEADER + X.vcf_line(1, 100, "w", info="END=%d" % ((1 << 29) + 1)) + X.vcf_line(1, (1 << 30) + 7, "big", info="END=3000000000") \
        + X.vcf_line(2, 9, "other", info="END=%d" % ((1 << 32) - 2))
    for name in ("already_sorted", "equal_keys", "undeclared_contig"):
        texts["sorted_" + name] = X.sorted_text(X.ORDERS[name])
    rows += [vcf_row(texts[name]) for name in sorted(texts)]
    rows.append(vcf_row(X.TEXTS["many_short_lines"], payload=97))       # many members, lines across them
    shares, weight = [[] for _ in range(SHARES)], [0] * SHARES
    for row, n in sorted(rows, key=lambda r: -r[1]):                    # a table of n rows costs n^2 / 2 folds of a row: the largest first
        k = weight.index(min(weight))
        shares[k].append(row)
        weight[k] += n * n + 1000
    return ["\n".join(share) + "\n" for share in shares], len(rows), sum(2 * (n + 1) for _row, n in rows)


def test_index_fold_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_csi_fold")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_csi_fold_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    texts, n_cases, n_folds = cases_text()
    runs = []
    for k, text in enumerate(texts):                # host programs side by side: the cases are independent of each other
        cases = str(tmp_path / ("cases%d.txt" % k))
        with open(cases, "w") as f:
            f.write(text)
        runs.append(subprocess.Popen([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    got_cases = got_folds = 0
    for run in runs:
        out, err = run.communicate(timeout=600)
        assert run.returncode == 0 and "AddressSanitizer" not in err and "runtime error" not in err, (out[-2000:], err[-3000:])
        lines = out.strip().splitlines()
        assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines[-5:]
        counts = [int(part.split()[0]) for part in lines[-2].split(", ")]
        got_cases, got_folds = got_cases + counts[0], got_folds + counts[1]
    assert got_cases == n_cases and got_folds == n_folds and n_cases > 45 and n_folds > 10000
