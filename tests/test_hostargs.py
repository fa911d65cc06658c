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
