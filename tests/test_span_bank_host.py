"""cordic_amd/csrc/cordic_span_bank.h, the host layer of the prefix-sum banks
(FM mixer banks, FM oscillator banks), as a function of the RULE and not of the
two rules it ships with: the cutter under a third, synthetic rule and a job
struct of the test's own, in a stand-alone C++ program with its own main under
the address and undefined-behaviour sanitizers.  No Python in the checked
process and no GPU, as in tests/test_bank_host.py.  And: launch 1 and the host
arithmetic exist once."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_span_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// a bank of the test's own: one output array of 4- or 2-byte samples
struct ToyJob { const uint32_t *d_fcw, *d_pm; int32_t *d_out; uint32_t *d_acc;
	uint64_t n; uint32_t phase0, reserved; };
struct ToyJob16 { const uint32_t *d_fcw, *d_pm; int16_t *d_out; uint32_t *d_acc;
	uint64_t n; uint32_t phase0, reserved; };
struct ToySpan { uint64_t fcw, pm, out, acc, n;
	uint32_t start, part0, idx, flags, phase0, pad; };
typedef JobView<ToyJob, ToyJob16> ToyJobs;
static void span_place(ToySpan *d, const ToyJob &jb, uint64_t at)
{
	d->out = (uintptr_t)jb.d_out + at;
}

constexpr SpanRule kToy = {8, 2, 4};

// addresses that are never dereferenced
template <typename J> static J job_at(size_t k, uint64_t n)
{
	J j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x100000u;
	j.d_fcw = (const uint32_t *)(base + 4 * (k % 4));
	j.d_pm = k % 2 ? (const uint32_t *)(base + 0x1000000000u) : nullptr;
	j.d_out = (decltype(j.d_out))(base + 0x2000000000u);
	j.d_acc = k % 3 ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}

template <typename J>
static void check_cut(const std::vector<J> &jobs, uint32_t base, uint32_t cap)
{
	const uint64_t es = sizeof *jobs.data()->d_out;
	std::vector<ToySpan> spans;
	uint32_t live = 0;
	span_cut(kToy, jobs.size(), ToyJobs(jobs.data()), base, cap, &spans, &live);
	EXPECT(spans.size() == span_count(kToy, jobs.size(), ToyJobs(jobs.data()), base, cap));
	size_t at = 0;
	uint32_t seen = 0;
	for (size_t k = 0; k < jobs.size(); k++) {
		const J &jb = jobs[k];
		if (!jb.n)
			continue;
		const size_t first = at;
		uint64_t done = 0, full = 0;
		while (done < jb.n) {
			EXPECT(at < spans.size());
			if (at >= spans.size())
				return;
			const ToySpan &s = spans[at];
			// the spans tile [0, n) in order, and none crosses the job's end
			EXPECT(s.fcw == (uintptr_t)jb.d_fcw + done * 4);
			EXPECT(s.pm == (jb.d_pm ? (uintptr_t)jb.d_pm + done * 4 : 0));
			EXPECT(s.out == (uintptr_t)jb.d_out + done * es);
			EXPECT(s.acc == (uintptr_t)jb.d_acc);
			EXPECT(s.phase0 == jb.phase0 && s.pad == 0);
			EXPECT(s.n >= 1 && s.n <= jb.n - done);
			EXPECT(s.start == seen && s.part0 == first && s.idx == at - first);
			const bool is_first = done == 0, is_last = done + s.n == jb.n;
			EXPECT(s.flags == ((is_first ? kSpanFirst : 0u) | (is_last ? kSpanLast : 0u)));
			if (!is_last) {		// whole units, all of one length
				EXPECT(s.n % kToy.unit == 0);
				EXPECT(full == 0 || s.n == full);
				full = s.n;
			} else {
				EXPECT(full == 0 || s.n <= full);
			}
			if (full) {		// the base length, or a power-of-two multiple
				const uint64_t u = full / kToy.unit;
				EXPECT(u >= base && u % base == 0 && !((u / base) & (u / base - 1)));
			}
			done += s.n;
			at++;
		}
		EXPECT(done == jb.n);
		EXPECT(at - first <= cap);
		// doubled only as far as the cap asks
		const uint64_t nu = span_units_of(kToy, jb.n);
		const uint64_t uj = span_job_units(kToy, jb.n, base, cap);
		EXPECT(at - first == (nu + uj - 1) / uj);
		EXPECT(uj == base || (nu + uj / 2 - 1) / (uj / 2) > cap);
		seen++;
	}
	EXPECT(at == spans.size() && seen == live);
}

template <typename J> static void check_container()
{
	const uint64_t lens[] = {0, 1, 7, 8, 9, 16, 17, 33, 65};
	std::vector<J> jobs;
	for (size_t k = 0; k < sizeof lens / sizeof *lens; k++)
		jobs.push_back(job_at<J>(k, lens[k]));
	const uint32_t cap = span_forced_cap(kToy, nullptr);
	EXPECT(cap == 2);
	for (uint32_t base = 1; base <= kToy.max_units; base *= 2) {
		check_cut(jobs, base, cap);
		check_cut(jobs, base, 1);
	}
	check_cut(std::vector<J>(), 1, cap);
}

int main()
{
	check_container<ToyJob>();
	check_container<ToyJob16>();
	EXPECT(ToyJobs((const ToyJob *)nullptr).esize() == 4);
	EXPECT(ToyJobs((const ToyJob16 *)nullptr).esize() == 2 && ToyJobs(nullptr).none());
	// by hand: 65 samples are 9 units; at most 2 spans: 8 units and 1 sample
	const ToyJob j = job_at<ToyJob>(1, 65);
	std::vector<ToySpan> s;
	uint32_t live = 0;
	span_cut(kToy, 1, ToyJobs(&j), 1, 2, &s, &live);
	EXPECT(live == 1 && s.size() == 2 && s[0].n == 64 && s[1].n == 1);
	EXPECT(s[0].flags == kSpanFirst && s[1].flags == kSpanLast && s[1].idx == 1);
	EXPECT(s[1].out == (uintptr_t)j.d_out + 256 && s[1].pm == (uintptr_t)j.d_pm + 256);
	EXPECT(span_units_of(kToy, 0) == 0 && span_units_of(kToy, 8) == 1
		&& span_units_of(kToy, 9) == 2);
	// the rule's own bounds in the knobs and in the base length
	EXPECT(span_forced_cap(kToy, "1") == 1 && span_forced_cap(kToy, "2") == 2);
	EXPECT(span_forced_cap(kToy, "3") == 2 && span_forced_cap(kToy, "0") == 2);
	EXPECT(span_forced_base(kToy, "4", 1) == 4 && span_forced_base(kToy, "8", 1) == 1);
	EXPECT(span_forced_base(kToy, "3", 2) == 2 && span_forced_base(kToy, nullptr, 2) == 2);
	EXPECT(span_base_units(kToy, ~(uint64_t)0, 1, 1) == 4);
	EXPECT(span_base_units(kToy, 0, 256, 2) == 1 && span_base_units(kToy, 4096, 256, 2) == 2);
	if (!failures)
		std::printf("span bank ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_cutter_under_a_third_rule_and_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "span_bank.cpp", tmp_path / "span_bank"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "span bank ok" in r.stdout


def test_launch_1_and_the_span_arithmetic_are_shared_not_pasted():
    """one reduce kernel over a span table among the sources, launched by both
    bank units; no cutter, span count or per-job span length in a bank's own
    header"""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip", ".cpp")):
            continue
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w*reduce)\s*\(([^)]*)\)", code):
            # (the single call's fm_reduce takes one array, not a span table)
            if re.search(r"\*\s*(__restrict__\s+)?spans\b", m.group(2)):
                found.append((name, m.group(1)))
    assert found == [("cordic_span_reduce.h", "span_reduce")], found
    for unit, inst in (("cordic_fm_mix_bank.hip", "span_reduce<MixSpan, 256>"),
                       ("cordic_table_fm_bank.hip", "span_reduce<FmSpan, 1024>")):
        body = open(os.path.join(CSRC, unit)).read()
        assert '#include "cordic_span_reduce.h"' in body, unit
        assert len(re.findall(r"hipLaunchKernelGGL\(\(%s\)" % re.escape(inst), body)) == 1, unit
        assert "__shfl_xor" not in re.sub(r"//[^\n]*", "", body), unit
    for head in ("cordic_fm_mix_bank.h", "cordic_table_fm_bank.h"):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, head)).read())
        assert '#include "cordic_span_bank.h"' in text, head
        assert not re.search(r"\b\w+_(cut|count_spans|job_passes|job_tiles)\s*\([^;{]*\)\s*\{",
                             text), head
        assert "strtol" not in text and "getenv" not in text, head
    text = open(os.path.join(CSRC, "cordic_span_bank.h")).read()
    assert "#include <hip" not in text
    for fn in ("span_units_of", "span_job_units", "span_count", "span_forced_cap",
               "span_base_units", "span_forced_base", "span_cut", "bank_jobs_valid"):
        assert len(re.findall(r"\binline\s+\w+\s+%s\s*\(" % fn, text)) == 1, fn
    stamp = open(os.path.join(ROOT, "tools", "build_stamp.py")).read()
    assert "cordic_span" not in stamp
