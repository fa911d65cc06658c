"""cordic_amd/csrc/cordic_bank_host.h: the overlap rule over sorted ranges, the
tile-length rule and the power-of-two knob that the creates of the job sets and
of the two FM banks share, in a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU, no Python in the checked process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "cordic_bank_host.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

struct R { uint64_t addr, bytes; bool out; };

// (addresses that are never dereferenced)
template <size_t N> static bool clear(const R (&r)[N], bool backwards = false)
{
	BankRanges b;
	for (size_t i = 0; i < N; i++) {
		const R &a = r[backwards ? N - 1 - i : i];
		EXPECT(b.add(a.addr, a.bytes, a.out));
	}
	return b.outputs_clear();
}

int main()
{
	const uint64_t x = 0x1000, y = 0x2000, m = 0x3000, f = 0x3100, n = 0x100;

	{	// the empty set
		BankRanges b;
		EXPECT(b.outputs_clear());
	}
	{	// disjoint ranges touching end to start: m ends where f begins
		const R r[] = {{x, n, false}, {y, n, false}, {m, n, true}, {f, n, true},
			{f + n, 4, true}, {f + n + 4, n, false}};
		EXPECT(clear(r) && clear(r, true));
	}
	{	// output over output by one byte
		const R r[] = {{m, n + 1, true}, {f, n, true}};
		EXPECT(!clear(r) && !clear(r, true));
		const R whole[] = {{m, n, true}, {m, n, true}};
		EXPECT(!clear(whole));
	}
	{	// output beginning one byte before an input's end
		const R r[] = {{x, n, false}, {x + n - 1, 8, true}};
		EXPECT(!clear(r) && !clear(r, true));
	}
	{	// output ending exactly at an input's start, and one byte further
		const R r[] = {{x, n, false}, {x - 8, 8, true}};
		EXPECT(clear(r) && clear(r, true));
		const R over[] = {{x, n, false}, {x - 8, 9, true}};
		EXPECT(!clear(over) && !clear(over, true));
	}
	{	// a 4-byte output inside an input, at its start, inside an output
		const R r[] = {{x, n, false}, {x + 20, 4, true}};
		EXPECT(!clear(r) && !clear(r, true));
		const R at0[] = {{x, n, false}, {x, 4, true}};
		EXPECT(!clear(at0) && !clear(at0, true));
		const R in_out[] = {{m, n, true}, {m + n - 4, 4, true}};
		EXPECT(!clear(in_out) && !clear(in_out, true));
	}
	{	// inputs aliasing inputs, wholly and partly; an output clear of them
		const R r[] = {{x, n, false}, {x, n, false}, {x + 4, n, false},
			{x + n - 1, n, false}, {m, n, true}};
		EXPECT(clear(r) && clear(r, true));
	}
	{	// a long input in front still covers an output behind a short one
		const R r[] = {{x, 0x1000, false}, {x + 8, 8, false}, {x + 0x800, 4, true}};
		EXPECT(!clear(r) && !clear(r, true));
	}
	{	// one fixed case in two orders of adding
		const R a[] = {{x, n, false}, {m, n, true}, {y, n, false}, {y + n - 4, 4, true}};
		const R b[] = {{y + n - 4, 4, true}, {y, n, false}, {m, n, true}, {x, n, false}};
		EXPECT(!clear(a) && !clear(b));
		const R c[] = {{x, n, false}, {m, n, true}, {y, n, false}, {y + n, 4, true}};
		const R d[] = {{y + n, 4, true}, {m, n, true}, {y, n, false}, {x, n, false}};
		EXPECT(clear(c) && clear(d));
	}
	{	// an address wrap is reported, and the range is not taken
		const uint64_t top = ~(uint64_t)0;
		BankRanges b;
		EXPECT(b.add(top - 8, 8, true));	// ends at the last address
		EXPECT(!b.add(top - 8, 9, true));
		EXPECT(!b.add(top, 1, false));
		EXPECT(!b.add(8, top - 7, true));
		EXPECT(b.add(8, top - 8 - 8 - 8, false));
		EXPECT(b.outputs_clear());
	}

	// the pass rule, demodulation bank: 8 blocks per CU, passes of 256 vectors,
	// at most 8 -- 256 CUs: total / 8192 / 256
	const int cuses[] = {256, 0, -1};
	for (int cus : cuses) {
		EXPECT(bank_passes(0, cus, 8, 256, 8) == 1);
		EXPECT(bank_passes(4194303, cus, 8, 256, 8) == 1);
		EXPECT(bank_passes(4194304, cus, 8, 256, 8) == 2);
		EXPECT(bank_passes(8388607, cus, 8, 256, 8) == 2);
		EXPECT(bank_passes(8388608, cus, 8, 256, 8) == 4);
		EXPECT(bank_passes(16777215, cus, 8, 256, 8) == 4);
		EXPECT(bank_passes(16777216, cus, 8, 256, 8) == 8);
		EXPECT(bank_passes(~(uint64_t)0, cus, 8, 256, 8) == 8);
		EXPECT(bank_tile_room(8192 * 5 + 8191, cus, 8) == 5);
	}
	EXPECT(bank_tile_room(1000, 5, 2) == 25 && bank_tile_room(39, 5, 2) == 0);
	// ... mixer bank: 4 blocks per CU, passes counted singly, at most 2^20
	const uint32_t mx = 1u << 20;
	EXPECT(bank_passes(0, 256, 4, 1, mx) == 1);
	EXPECT(bank_passes(8191, 256, 4, 1, mx) == 1);
	EXPECT(bank_passes(8192, 256, 4, 1, mx) == 2);
	EXPECT(bank_passes(65536, 256, 4, 1, mx) == 16);
	EXPECT(bank_passes(65536, 64, 4, 1, mx) == 64);
	EXPECT(bank_passes(~(uint64_t)0, 1, 4, 1, mx) == mx);

	// the knob with maximum 8
	const char *keep[] = {nullptr, "", "x", "0", "-2", "3", "16"};
	for (const char *e : keep)
		EXPECT(bank_forced_passes(e, 8, 4) == 4 && bank_forced_passes(e, 8, 1) == 1);
	EXPECT(bank_forced_passes("1", 8, 4) == 1 && bank_forced_passes("2", 8, 4) == 2);
	EXPECT(bank_forced_passes("4", 8, 1) == 4 && bank_forced_passes("8", 8, 4) == 8);
	if (!failures)
		std::printf("bank host ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_shared_bank_rules_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "bank_host.cpp", tmp_path / "bank_host"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "bank host ok" in r.stdout


def test_the_header_is_plain_cxx_and_the_banks_use_it():
    """only standard headers; the two FM banks' headers include it and carry no
    copy of the sorted scan"""
    text = open(os.path.join(CSRC, "cordic_bank_host.h")).read()
    incs = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(incs) == ["<algorithm>", "<cstddef>", "<cstdint>", "<cstdlib>",
                            "<vector>"]
    assert "any_end" in text
    for unit in ("cordic_fm_demod_bank.h", "cordic_fm_mix_bank.h"):
        body = open(os.path.join(CSRC, unit)).read()
        assert '#include "cordic_bank_host.h"' in body, unit
        assert "any_end" not in body, unit
