"""Makes tests/golden/classify_cases.json.gz: what the reference's scripts/sv_classifier.py gives for the corpus of
tests/classifycases.py.

DEVELOPMENT MACHINE ONLY, like make_golden_paste.py: it needs the reference checkout ($SVTYPER_REFERENCE, read-only), numpy and
scipy.  No reference source is copied: the Python 2 script is read from there, converted by the stdlib lib2to3 in memory and
exec'd (make_golden_paste.load_script), with
  * time.strftime fixed (FILE_DATE);
  * stats.linregress wrapped, so that every (slope, r) it returns is recorded;
  * sv_classify driven directly with file objects, so the AttributeError the script ends with when -e is absent plays no part;
    the annotation dictionary is built here the way the script's main() builds it;
  * stdout, stderr and the exit status captured.
A case's record: its name, `stdout` with status 0, or the status, the exception's type, the text on stderr and the `stdout`
written before the script died; and the regressions the script ran, in order.  The inputs are not stored: tests/classifycases.py rebuilds them.

MARGIN: every recorded r**2 and signed slope lies at least 1e-6 (relative) from its threshold, or the generator refuses: the
goldens then hold for any summation order of the regression, whose results agree to 1e-9 and better.

    python tests/golden/make_golden_classify.py [--check]   # --check: compare with the committed file, write nothing
"""
import gzip
import io
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import classifycases  # noqa: E402
from make_golden_paste import FILE_DATE, load_script, run  # noqa: E402

OUT = os.path.join(HERE, "classify_cases.json.gz")
MARGIN = 1e-6


def annotated_elements(path):
    elements = {}
    with open(path) as f:
        for row in f:
            v = row.rstrip().split("\t")
            if len(v) < 4:
                continue
            elements.setdefault(v[0], []).append([int(v[1]), int(v[2])] + v[3:])
    return elements


def expected(case, script, recorded):
    del recorded[:]
    with tempfile.TemporaryDirectory() as tmp:
        vcf, gender, exclude, annotation = classifycases.write_case(case, tmp)
        files = [open(p, newline="") if p is not None else None for p in (vcf, gender, exclude)]
        elements = annotated_elements(annotation) if annotation is not None else None
        o = case["options"]
        out, err, status, kind = run(lambda: script.sv_classify(files[0], files[1], files[2], elements, o["f_overlap"], o["slope_threshold"],
                                                                o["rsquared_threshold"]))
        for f in files:
            if f is not None:
                f.close()
    for slope, r, svtype in recorded:
        for value, threshold in ((r * r, o["rsquared_threshold"]), (-slope if svtype == "DEL" else slope, o["slope_threshold"])):
            distance = abs(value - threshold) / abs(threshold) if threshold else abs(value - threshold)
            assert distance >= MARGIN, "%s: %r lies within the margin of its threshold %r" % (case["name"], value, threshold)
    record = dict(name=case["name"], regressions=[[slope, r] for slope, r, _ in recorded])
    record["expected"] = dict(status=status, exception=kind, stderr=err, stdout=out) if status else dict(status=0, stdout=out)
    return record


def make():
    script = load_script("sv_classifier.py")
    script.time = types.SimpleNamespace(strftime=lambda fmt: FILE_DATE)
    recorded = []
    linregress = script.stats.linregress

    def recording(rd):
        result = linregress(rd)
        # (the type of the line is not the regression's business: the caller's frame holds it)
        svtype = sys._getframe(1).f_locals["var"].info["SVTYPE"]
        recorded.append((float(result[0]), float(result[2]), svtype))
        return result

    script.stats = types.SimpleNamespace(linregress=recording)
    return dict(file_date=FILE_DATE, cases=[expected(case, script, recorded) for case in classifycases.cases()])


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
