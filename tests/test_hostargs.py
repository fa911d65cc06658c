"""cordic_amd/csrc/cordic_hostargs.h: the range checks and the grid cap that the
FM units' entry points share, in a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU, no Python in the checked process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include "cordic_hostargs.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// the I/Q call check at n = 64 on samples of es bytes: every array 1 KiB apart
// on the 16-byte grid, the words and the workspace behind them
static void iq_calls(const size_t es)
{
	alignas(16) static unsigned char a[16384];
	const size_t n = 64, wb = 256;
	unsigned char *f = a + 1024, *m = a + 2048, *x = a + 3072, *y = a + 4096,
		*o0 = a + 5120, *o1 = a + 6144, *acc = a + 7168, *last = a + 7184,
		*w = a + 8192;
	auto ok = [&](const void *pacc, const void *plast, const void *pf, const void *pm,
			const void *px, const void *py, const void *p0, const void *p1,
			const void *pw, size_t nn = 64) {
		return iq_call_ok(nn, pacc, plast, pf, pm, px, py, p0, p1, es, pw, wb);
	};
	EXPECT(ok(acc, last, f, m, x, y, o0, o1, w));
	EXPECT(ok(acc, last, f, m, x, x, o0, o1, w));		// x aliased to y
	EXPECT(ok(acc, last, f, nullptr, x, y, o0, o1, w));	// the optional ones
	EXPECT(ok(nullptr, last, f, m, x, y, o0, o1, w));
	EXPECT(ok(acc, nullptr, f, m, x, y, o0, o1, w));
	EXPECT(ok(nullptr, nullptr, f, nullptr, x, y, o0, o1, w));
	// each required pointer
	EXPECT(!ok(acc, last, nullptr, m, x, y, o0, o1, w));
	EXPECT(!ok(acc, last, f, m, nullptr, y, o0, o1, w));
	EXPECT(!ok(acc, last, f, m, x, nullptr, o0, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, nullptr, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, nullptr, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1, nullptr));
	// a word pointer off the 4-byte grid
	EXPECT(!ok(acc + 2, last, f, m, x, y, o0, o1, w));
	EXPECT(!ok(acc, last + 1, f, m, x, y, o0, o1, w));
	EXPECT(!ok(acc, last, f + 2, m, x, y, o0, o1, w));
	EXPECT(!ok(acc, last, f, m + 1, x, y, o0, o1, w));
	// a sample pointer off the grid of es, and on it
	const size_t off = es / 2;
	EXPECT(!ok(acc, last, f, m, x + off, y, o0, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y + off, o0, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0 + off, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1 + off, w));
	EXPECT(ok(acc, last, f, m, x + es, y + es, o0 + es, o1 + es, w));
	// d_work off the 16-byte grid
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1, w + 8));
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1, w + 4));
	// an output beginning one element inside each kind of input
	EXPECT(!ok(acc, last, f, m, x, y, f + 4 * (n - 1), o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, m + 4 * (n - 1), w));
	EXPECT(!ok(acc, last, f, m, x, y, x + es * (n - 1), o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, y + es * (n - 1), w));
	// ... and touching it, one element on
	EXPECT(ok(acc, last, f, m, x, y, f + 4 * n, o1, w));
	EXPECT(ok(acc, last, f, m, x, y, o0, m + 4 * n, w));
	EXPECT(ok(acc, last, f, m, x, y, x + es * n, o1, w));
	EXPECT(ok(acc, last, f, m, x, y, o0, y + es * n, w));
	// the two outputs over each other by one element, and touching
	EXPECT(!ok(acc, last, f, m, x, y, o0, o0 + es * (n - 1), w));
	EXPECT(ok(acc, last, f, m, x, y, o0, o0 + es * n, w));
	// d_last inside omag, and just behind it
	EXPECT(!ok(acc, o0 + es * n - 4, f, m, x, y, o0, o1, w));
	EXPECT(ok(acc, o0 + es * n, f, m, x, y, o0, o1, w));
	EXPECT(!ok(o1 + 4, last, f, m, x, y, o0, o1, w));	// d_acc inside ofreq
	EXPECT(!ok(acc, x + 4, f, m, x, y, o0, o1, w));		// d_last inside an input
	EXPECT(!ok(acc, acc, f, m, x, y, o0, o1, w));		// d_acc == d_last
	EXPECT(ok(acc, acc + 4, f, m, x, y, o0, o1, w));
	// the work_bytes of d_work reach the first output, and end where it begins
	EXPECT(!ok(acc, last, f, m, x, y, w + wb - 16, o1, w));
	EXPECT(ok(acc, last, f, m, x, y, w + wb, o1, w));
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1, o0 - wb + 16));
	EXPECT(ok(acc, last, f, m, x, y, o0, o1, o0 - wb));
	// the longest call, and one sample more (nothing is dereferenced)
	EXPECT(!ok(nullptr, nullptr, f, nullptr, x, x, o0, o0, w, (~(size_t)0 >> 4) + 1));
	EXPECT(!ok(acc, last, f, m, x, y, o0, o1, w, (~(size_t)0 >> 4) + 1));
}

// call_span against the two formulas the launchers had, written out
static void spans()
{
	const size_t big = ~(size_t)0 >> 4;
	const size_t ns[] = {1, 3, 4, 5, 1019, 1020, 1021, 1023, 1024, 1025, 2039, 2040, 2041,
		2048, 4097, 3 * 1020, 3 * 1020 + 1, ((size_t)1 << 20) + 7, (size_t)1 << 28, big};
	const size_t caps[] = {1, 2, 3, 7, 1024, 4096};
	for (size_t n : ns)
		for (size_t cap : caps) {
			{	// the mixer's
				const size_t npass = (n + 1024 - 1) / 1024;
				const size_t per = (npass + cap - 1) / cap;
				const size_t span = per * 1024;
				const size_t grid = (npass + per - 1) / per;
				const CallSpan cs = call_span(n, cap, 1024, 0);
				EXPECT(cs.span == span && cs.grid == grid);
				EXPECT(cs.grid <= cap);
				EXPECT((cs.grid - 1) * cs.span < n && (n - 1) / cs.span < cs.grid);
			}
			{	// the receiver's
				const size_t yield1 = 1020;
				const size_t npass = (n + yield1 - 1) / yield1;
				const size_t per = (npass + cap - 1) / cap;
				const size_t span = per * 1024 - 4;
				const size_t grid = (n + span - 1) / span;
				const CallSpan cs = call_span(n, cap, 1024, 4);
				EXPECT(cs.span == span && cs.grid == grid);
				EXPECT(cs.grid <= cap);
				EXPECT((cs.grid - 1) * cs.span < n && (n - 1) / cs.span < cs.grid);
			}
		}
}

int main()
{
	static unsigned char a[4096];
	const size_t n = 64, b = n * 4;
	// (x and y with room around them; m begins where y ends, f where m ends)
	unsigned char *x = a, *y = a + 512, *m = a + 768, *f = a + 1024, *l = a + 1280,
		*w = a + 1284;

	{	// disjoint ranges, touching end to start
		const Range out[4] = {range_of(m, b), range_of(f, b), range_of(l, 4),
			range_of(w, 64)};
		const Range in[2] = {range_of(x, b), range_of(y, b)};
		EXPECT(!outputs_overlap(out, in));
		EXPECT(!outputs_overlap(out, in, true));
		EXPECT(hits(out[0], out[0]) && !hits(out[0], out[1]) && !hits(in[1], out[0]));
	}
	{	// inputs may lie over each other
		const Range out[1] = {range_of(m, b)};
		const Range in[2] = {range_of(x, b), range_of(x + 4, b)};
		EXPECT(!outputs_overlap(out, in));
	}
	{	// output over output, by one byte and whole
		const Range in[1] = {range_of(x, b)};
		const Range o1[2] = {range_of(m, b + 1), range_of(f, b)};
		const Range o2[2] = {range_of(m, b), range_of(m, b)};
		const Range o3[3] = {range_of(m, b), range_of(f, b), range_of(f + b - 1, 4)};
		EXPECT(outputs_overlap(o1, in));
		EXPECT(outputs_overlap(o2, in));
		EXPECT(outputs_overlap(o3, in));
	}
	{	// output over input by one byte at either end, and clear of it
		const Range in[2] = {range_of(x, b), range_of(y, b)};
		const Range front[1] = {range_of(y - 8, 9)};	// its last byte is y[0]
		const Range back[1] = {range_of(y + b - 1, 8)};	// its first is y's last
		const Range before[1] = {range_of(y - 8, 8)};
		const Range behind[1] = {range_of(y + b, 8)};
		const Range both[2] = {range_of(y - 8, 8), range_of(y + b, 8)};
		EXPECT(outputs_overlap(front, in));
		EXPECT(outputs_overlap(back, in));
		EXPECT(!outputs_overlap(before, in) && !outputs_overlap(behind, in));
		EXPECT(!outputs_overlap(both, in));
		const Range second[2] = {range_of(m, b), range_of(x + b - 1, 8)};
		EXPECT(outputs_overlap(second, in));
	}
	{	// a NULL optional array is empty, wherever address 0 + bytes would reach
		const Range none = range_of(nullptr, ~(size_t)0 >> 1);
		EXPECT(none.bytes == 0 && none.lo == 0);
		const Range out[3] = {range_of(m, b), none, none};
		const Range in[3] = {range_of(x, b), none, range_of(y, b)};
		EXPECT(!outputs_overlap(out, in));
		const Range all[2] = {range_of(a, sizeof a), none};
		EXPECT(outputs_overlap(all, in));
	}
	{	// a zero-length call: every array on the same address
		const Range out[3] = {range_of(x, 0), range_of(x, 0), range_of(l, 4)};
		const Range in[2] = {range_of(x, 0), range_of(x, 0)};
		EXPECT(!outputs_overlap(out, in));
		const Range inside[1] = {range_of(x + 8, 0)};
		const Range around[1] = {range_of(x, b)};
		EXPECT(!outputs_overlap(inside, around) && !hits(around[0], inside[0]));
	}
	{	// the exact in-place pair, allowed and disallowed
		const Range out[2] = {range_of(x, b), range_of(l, 4)};
		const Range in[2] = {range_of(x, b), range_of(y, b)};
		EXPECT(outputs_overlap(out, in));
		EXPECT(outputs_overlap(out, in, false));
		EXPECT(!outputs_overlap(out, in, true));
		// ... one element on, either way: not the in-place form
		const Range on[2] = {range_of(x + 4, b), range_of(l, 4)};
		const Range back[2] = {range_of(x, b), range_of(l, 4)};
		const Range in4[2] = {range_of(x + 4, b), range_of(y + 4, b)};
		EXPECT(outputs_overlap(on, in, true));
		EXPECT(outputs_overlap(back, in4, true));
		// ... only out[0] on in[0]: not out[0] on in[1], not out[1] on in[0]
		const Range in_swapped[2] = {range_of(y, b), range_of(x, b)};
		const Range out_swapped[2] = {range_of(l, 4), range_of(x, b)};
		EXPECT(outputs_overlap(out, in_swapped, true));
		EXPECT(outputs_overlap(out_swapped, in, true));
		// ... and it excuses nothing else
		const Range two[2] = {range_of(x, b), range_of(x, b)};
		EXPECT(outputs_overlap(two, in, true));
	}
	{	// the block cap
		const char *name = "CORDIC_HOSTARGS_TEST_BLOCKS";
		unsetenv(name);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "0", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "-3", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "seven", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "1", 1);
		EXPECT(env_block_cap(name, 2048) == 1);
		setenv(name, "37", 1);
		EXPECT(env_block_cap(name, 2048) == 37);
		setenv(name, "2047", 1);
		EXPECT(env_block_cap(name, 2048) == 2047);
		setenv(name, "2048", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "100000", 1);
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "99999999999999999999999", 1);	// strtol saturates
		EXPECT(env_block_cap(name, 2048) == 2048);
		setenv(name, "5", 1);		// read at every call
		EXPECT(env_block_cap(name, 2048) == 5);
		EXPECT(env_block_cap(name, 3) == 3);
		unsetenv(name);
		EXPECT(env_block_cap(name, 3) == 3);
	}
	iq_calls(4);
	iq_calls(2);
	spans();
	if (!failures)
		std::printf("hostargs ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_shared_host_checks_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "hostargs.cpp", tmp_path / "hostargs"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "cordic_amd", "csrc"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "hostargs ok" in r.stdout


def test_the_header_is_plain_cxx_without_the_hip_headers(tmp_path):
    """only <cstddef>, <cstdint>, <cstdlib>: g++ with no include path but its own"""
    text = open(os.path.join(ROOT, "cordic_amd", "csrc", "cordic_hostargs.h")).read()
    incs = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(incs) == ["<cstddef>", "<cstdint>", "<cstdlib>"]
    for unit in ("cordic_fm_demod.hip", "cordic_fm_mix.hip", "cordic_table_fm.hip"):
        body = open(os.path.join(ROOT, "cordic_amd", "csrc", unit)).read()
        assert '#include "cordic_hostargs.h"' in body, unit
        assert "struct Range" not in body, unit
