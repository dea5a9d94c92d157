"""Makes tests/golden/modify_header_cases.json.gz: what the reference's scripts/vcf_modify_header.py gives for the corpus of
tests/modifyheadercases.py.

DEVELOPMENT MACHINE ONLY, like make_golden_paste.py: it needs the reference checkout ($SVTYPER_REFERENCE, read-only).  No
reference source is copied: the Python 2 script is read from there, converted by the stdlib lib2to3 in memory and exec'd
(make_golden_paste.load_script), with
  * time.strftime fixed (FILE_DATE);
  * mod_header, its primary function, driven directly with the case's options and file, opened without newline translation;
  * stdout, stderr and the exit status captured.
A case's record: its name, and `stdout` with status 0, or the status, the exception's type, the text on stderr and the `stdout`
written before the script died.  The inputs are not stored: tests/modifyheadercases.py rebuilds them.

    python tests/golden/make_golden_modify_header.py [--check]   # --check: compare with the committed file, write nothing
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
import modifyheadercases  # noqa: E402
from make_golden_paste import FILE_DATE, load_script, run  # noqa: E402

OUT = os.path.join(HERE, "modify_header_cases.json.gz")


def expected(case, script):
    with tempfile.TemporaryDirectory() as tmp:
        with open(modifyheadercases.write_case(case, tmp), newline="") as f:
            out, err, status, kind = run(lambda: script.mod_header(case["vcf_id"], case["category"], case["type"], case["number"],
                                                                   case["description"], f))
    record = dict(name=case["name"])
    record["expected"] = dict(status=status, exception=kind, stderr=err, stdout=out) if status else dict(status=0, stdout=out)
    return record


def make():
    script = load_script("vcf_modify_header.py")
    script.time = types.SimpleNamespace(strftime=lambda fmt: FILE_DATE)
    return dict(file_date=FILE_DATE, cases=[expected(case, script) for case in modifyheadercases.cases()])


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
