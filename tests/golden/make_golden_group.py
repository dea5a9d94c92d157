"""Makes tests/golden/group_cases.json.gz: what the reference's scripts/vcf_group_multiline.py gives for the corpus of
tests/groupcases.py.

DEVELOPMENT MACHINE ONLY, like make_golden_paste.py: it needs the reference checkout ($SVTYPER_REFERENCE, read-only).  No
reference source is copied: the Python 2 script is read from there, converted by the stdlib lib2to3 in memory and exec'd
(make_golden_paste.load_script, which also stands in for the `pysam` the script imports and never uses), with
  * time.strftime fixed (FILE_DATE);
  * sv_genotype, its primary function, driven directly with the case's file, opened without newline translation;
  * stdout, stderr and the exit status captured.
A case's record: its name, and `stdout` with status 0, or the status, the exception's type, the text on stderr and the `stdout`
written before the script died.  The inputs are not stored: tests/groupcases.py rebuilds them.

The script runs under Python 3 here: the corpus holds no token that Python 2 and 3 read differently (tests/groupcases.py).

    python tests/golden/make_golden_group.py [--check]   # --check: compare with the committed file, write nothing
"""
import gzip
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import groupcases  # noqa: E402
from make_golden_paste import FILE_DATE, load_script, run  # noqa: E402

OUT = os.path.join(HERE, "group_cases.json.gz")


def expected(case, script):
    with tempfile.TemporaryDirectory() as tmp:
        with open(groupcases.write_case(case, tmp), newline="") as f:
            out, err, status, kind = run(lambda: script.sv_genotype(f))
    record = dict(name=case["name"])
    record["expected"] = dict(status=status, exception=kind, stderr=err, stdout=out) if status else dict(status=0, stdout=out)
    return record


def make():
    script = load_script("vcf_group_multiline.py")
    script.time = types.SimpleNamespace(strftime=lambda fmt: FILE_DATE)
    return dict(file_date=FILE_DATE, cases=[expected(case, script) for case in groupcases.cases()])


def main():
    made = json.dumps(make(), sort_keys=True, separators=(",", ":")).encode()
    if "--check" in sys.argv[1:]:
        with gzip.open(OUT, "rb") as f:
            same = f.read() == made
        print("%s: %s" % (OUT, "reproduced" if same else "DIFFERS"))
        return 0 if same else 1
    with open(OUT, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
        z.write(made)
    print("%s: %d cases, %d bytes" % (OUT, len(json.loads(made)["cases"]), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
