"""Makes tests/golden/paste_cases.json.gz: what the reference's scripts/vcf_paste.py and scripts/vcf_allele_freq.py give for the
corpus of tests/pastecases.py.

DEVELOPMENT MACHINE ONLY, like make_golden.py: it needs the reference checkout ($SVTYPER_REFERENCE, read-only).  No reference
source is copied: the two Python 2 scripts are read from there, converted by the stdlib lib2to3 in memory and exec'd, with
  * a stand-in `pysam` module (vcf_allele_freq.py imports it and never uses it);
  * the module-level name `str` bound to Python 2's str(float) -- "%.12g", ".0" appended where that looks like an integer --
    since vcf_paste.py prints the -q QUAL through map(str, ...);
  * stdout, stderr and the exit status captured, and time.strftime fixed (FILE_DATE).
A case's record: its inputs and options as tests/pastecases.py built them, and `stdout` with status 0, or the status, the
exception's type and the text on stderr of the script that ended the run.

    python tests/golden/make_golden_paste.py [--check]      # --check: compare with the committed file, write nothing
"""
import contextlib
import gzip
import io
import json
import os
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pastecases  # noqa: E402

REFERENCE_ROOT = os.environ.get("SVTYPER_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "paste_cases.json.gz")
FILE_DATE = "20200229"


def py2_str(value=""):
    if isinstance(value, float):
        text = "%.12g" % value
        return text if any(c in text for c in ".en") else text + ".0"
    return str(value)


class _Kept(io.StringIO):
    """a stdout the script may close"""

    def close(self):
        pass


def load_script(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
        tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
        path = os.path.join(REFERENCE_ROOT, "scripts", name)
        with open(path) as f:
            source = f.read()
        source = str(tool.refactor_string(source if source.endswith("\n") else source + "\n", path))
    module = types.ModuleType("reference_" + name[:-3])
    module.__file__ = path
    module.str = py2_str
    saved = sys.modules.get("pysam")
    sys.modules["pysam"] = types.ModuleType("pysam")
    try:
        exec(compile(source, path, "exec"), module.__dict__)
    finally:
        if saved is None:
            del sys.modules["pysam"]
        else:
            sys.modules["pysam"] = saved
    return module


def run(call):
    """(stdout, stderr, status, the exception's type or None) of one script's primary function"""
    out, err = _Kept(), io.StringIO()
    status, kind = 0, None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            call()
        except SystemExit as e:
            status = e.code if isinstance(e.code, int) else 1
        except Exception as e:                      # (a traceback and status 1 in the script's own process)
            status, kind = 1, type(e).__name__
    return out.getvalue(), err.getvalue(), status, kind


def expected(case, paste_script, afreq_script):
    with tempfile.TemporaryDirectory() as tmp:
        master, paths = pastecases.write_case(case, tmp)
        files = [open(p) for p in paths]
        master_file = open(master) if master is not None else None
        out, err, status, kind = run(lambda: paste_script.svt_join(master_file, case["sum_quals"], files))
        for f in files + ([master_file] if master_file else []):
            f.close()
    if status == 0 and case["afreq"]:
        pasted = io.StringIO(out)
        out, err, status, kind = run(lambda: afreq_script.add_af(pasted))
    if status:
        return dict(status=status, exception=kind, stderr=err)
    return dict(status=0, stdout=out)


def make():
    paste_script, afreq_script = load_script("vcf_paste.py"), load_script("vcf_allele_freq.py")
    afreq_script.time = types.SimpleNamespace(strftime=lambda fmt: FILE_DATE)
    records = []
    for case in pastecases.cases():
        record = {k: case[k] for k in ("name", "master", "inputs", "sum_quals", "afreq")}
        record["expected"] = expected(case, paste_script, afreq_script)
        records.append(record)
    return dict(file_date=FILE_DATE, cases=records)


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
