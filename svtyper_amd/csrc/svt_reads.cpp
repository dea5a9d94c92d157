// svt_reads.cpp -- native BAM access + fragment summariser (include/svtyper_reads.h).
//
// Host-only C++ (no HIP): BAM/BAI reader over the BGZF layer of svt_bgzf_reader.h, with the fetch()/count() semantics the SVTyper path
// relies on (pysam's, as restated in svtyper_amd/bam.py), read-fragment assembly and split-read QC
// (svtyper/parsers.py:729-768, 891-1058 as restated in svtyper_amd/fragments.py) and the emission of
// svt_fragment summaries (svtyper_amd/geometry.py).  The Python modules are the portable
// implementation and the checker of this file (tests/test_native_reads.py compares the summaries
// byte for byte); this file exists because per-read Python objects, not the GPU, bound a real run.

#include <sys/mman.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/svtyper_reads.h"
#include "svt_bai_index.h"
#include "svt_bam_index.h"
#include "svt_bam_first_rules.h"
#include "svt_bam_sort_rules.h"
#include "svt_bcf.h"
#include "svt_bcf_text.h"
#include "svt_bgzf.h"
#include "svt_dump_rules.h"
#include "svt_error.h"
#include "svt_evidence_arena.h"
#include "svt_geometry_math.h"
#include "svt_host_cpus.h"
#include "svt_library_arena.h"
#include "svt_cram.h"
#include "svt_rans_batch.h"
#include "svt_record_rules.h"
#include "svt_tbx_index.h"
#include "svt_vcf_lines.h"
#include "svt_vcf_paste.h"
#include "svt_vcf_classify.h"
#include "svt_vcf_update_info.h"
#include "svt_vcf_group.h"

namespace {
using svt::fail;
using svt::guarded;
using svt::run_threads;
namespace rr = svt::rr;
using rr::clip32;
using rr::ld32;
}  // namespace

// The parts, in order: each needs only what stands in front of it.
#include "svt_bgzf_reader.h"           // FileMap, Bgzf and the host loop over a bgzf::MemberSet: this translation unit's BGZF layer
#include "svt_reads_handle.h"          // struct svt_bam, the verify scope, open / close / accessors
#include "svt_reads_records.h"         // Record, its tag walk, next_record, the pysam-style fetch
#include "svt_reads_fragments.h"       // Workspace, process_unit, evidence_unit, UnitReader
#include "svt_reads_pool.h"            // BufferPool, SummaryArena, svt_reads_trim
#include "svt_reads_summarise.h"       // svt_bam_summarise, svt_bam_evidence and their gather
#include "svt_reads_arena.h"           // svt::ew: the evidence arena's planner, host_units
#include "svt_reads_walk.h"            // the one-source walk on the host, its dump, their entry points
#include "svt_reads_bgzf_entries.h"    // svt_bgzf_inflate_host, _crc32_host, _deflate_host
#include "svt_reads_library.h"         // svt_bam_scan_library, svt::lw: the segmented library walk
#include "svt_reads_vcf_entries.h"     // svt_vcf_lines_host, _gather_host, _sort_order, svt_tbx_build: VCF text as lines, the .tbi fold
#include "svt_reads_bam_sort_entries.h" // svt_bam_spans_host, _sort_order_host, svt_bai_build: BAM records as spans, the .bai fold
#include "svt_reads_bcf_entries.h"     // svt_bcf_encode_host, svt_bcf_take, svt_bcf_text_host, svt_bcf_text_take: VCF text as a BCF stream and back
#include "svt_reads_paste_entries.h"   // svt_vcf_paste_host: per-sample VCFs joined by line number, AF and NSAMP
#include "svt_reads_cohort_entries.h"  // cohort_write, cohort_take: the writer's entry points of a rule over cohort lines
#include "svt_reads_classify_entries.h" // svt_vcf_classify_host, _write, _take: the read-depth classifier of DEL and DUP lines
#include "svt_reads_update_info_entries.h" // svt_vcf_update_info_host, _write, _take: PE, SR, SU and MSQ from the samples' evidence
#include "svt_reads_group_entries.h"  // svt_vcf_group_host, _write, _take: BND mates grouped in front of the paste
#include "svt_entry_cram.h"           // svt_rans_decode_host, svt_cram_decode_slice, svt_cram_take: the CRAM reader's native parts
