"""The corpus of svtyper_amd.modify_header, shared by tests/test_modify_header.py and tests/golden/make_golden_modify_header.py.
Everything is built in code and deterministic; inputs are not stored.

A case: name, vcf, and the script's options: vcf_id, category, type, number, description (None: not given).  What the
reference's scripts/vcf_modify_header.py gives for a case is in tests/golden/modify_header_cases.json.gz, by name.
"""
HEADER = ["##fileformat=VCFv4.1", "##fileDate=20190101", "##source=test", "##reference=ref.fa",
          '##FILTER=<ID=LOW,Description="Low quality">', '##FILTER=<ID=ODD,Description="a > inside, and a comma">',
          "##contig=<ID=1,length=249250621>",
          '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
          '##INFO=<ID=END,Number=1,Type=Integer,Description="End position">',
          '##INFO=<ID=NOTE,Number=.,Type=String,Description="one, two">',
          '##INFO=<ID=END,Number=2,Type=String,Description="declared again">',
          '##ALT=<ID=DEL,Description="Deletion">',
          '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">',
          '##FORMAT=<ID=GT,Number=2,Type=Integer,Description="not the script\'s">']
BODY = "1\t100\ta\tN\t<DEL>\t.\t.\tSVTYPE=DEL;END=200;UNDECLARED\tXX:GT\t5:0/1\t \n1\t 7\tb\tN\t<DEL>\tnot parsed\n\n#late\t\n"


def vcf(samples=("S0", "S1"), body=BODY, header=HEADER, chrom=True):
    columns = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] + (["FORMAT"] + list(samples) if samples else [])
    return "\n".join(list(header) + (["\t".join(columns)] if chrom else [])) + "\n" + body


def case(name, text, vcf_id=None, category=None, type=None, number=None, description=None):
    return dict(name=name, vcf=text, vcf_id=vcf_id, category=category, type=type, number=number, description=description)


def cases():
    out = [case("normalise_only", vcf()),
           case("info_new", vcf(), "MSQ", "INFO", "Float", "1", "Mean sample quality"),
           case("info_replaces", vcf(), "END", "INFO", "Integer", "1", "End, declared anew"),
           case("info_quoted_description", vcf(), "Q", "INFO", "String", ".", '"quoted"'),
           case("info_options_missing", vcf(), "X", "INFO"),
           case("format_new", vcf(), "SQ", "FORMAT", "Float", "1", "Sample quality"),
           case("format_declared_already", vcf(), "GQ", "FORMAT", "Float", "A", "ignored"),
           case("format_gt", vcf(), "GT", "FORMAT", "String", "9", "ignored: the script's GT stands"),
           case("filter_new", vcf(), "PASSED", "FILTER", None, None, "Passed all"),
           case("filter_declared_already", vcf(), "LOW", "FILTER", None, None, "ignored"),
           case("category_unknown", vcf(), "Z", "ALT", "String", "1", "no such category"),
           case("no_samples", vcf(samples=()), "MSQ", "INFO", "Float", "1", "Mean sample quality"),
           case("no_body", vcf(body=""), "MSQ", "INFO", "Float", "1", "Mean sample quality"),
           case("last_line_bare", vcf(body="1\t100\ta\tN\t<DEL>\t.\t.\tEND=3"), "MSQ", "INFO", "Float", "1", "d"),
           case("carriage_returns", vcf().replace("\n", "\r\n"), "LATE", "FILTER", None, None, "d"),
           case("error_no_chrom_line", vcf(chrom=False), "MSQ", "INFO", "Float", "1", "d")]
    assert len({c["name"] for c in out}) == len(out)
    return out


def write_case(c, directory):
    """the case's VCF under `directory`: its path"""
    import os
    path = os.path.join(directory, "calls.vcf")
    with open(path, "w", newline="") as f:
        f.write(c["vcf"])
    return path
