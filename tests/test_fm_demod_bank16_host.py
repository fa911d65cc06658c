"""cordic_amd/csrc/cordic_fm_demod_bank.h on 16-bit jobs: the validity check
and the cutter of cordic_demodbank_create16, which serve both job structs
through one implementation (DemodJobs), in a stand-alone program with its own
main under the address and undefined-behaviour sanitizers.  No GPU, no Python in
the checked process, nothing preloaded."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cordic_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cordic_fm_demod_bank.h"

using namespace cordic_amd;

static int failures;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); \
	failures++; } } while (0)

// addresses that are never dereferenced: job k's four arrays in four regions,
// at an element offset of k % 4 behind a 16-byte boundary
template <typename Job, typename E>
static Job job_at(size_t k, uint64_t n, bool last)
{
	Job j;
	std::memset(&j, 0, sizeof j);
	const uintptr_t base = 0x10000000u + (uintptr_t)k * 0x10000000u;
	const uintptr_t odd = sizeof(E) * (k % 4);
	j.d_xval = (const E *)(base + 0x2000000000u + odd);
	j.d_yval = (const E *)(base + 0x3000000000u + odd);
	j.d_omag = (E *)(base + 0x4000000000u + odd);
	j.d_ofreq = (E *)(base + 0x5000000000u + odd);
	j.d_last = last ? (uint32_t *)(0x6000000000u + 16 * k) : nullptr;
	j.n = n;
	j.phase0 = (uint32_t)(k * 0x9e3779b1u);
	return j;
}
static cordic_demod_job16 job16(size_t k, uint64_t n, bool last = true)
{
	return job_at<cordic_demod_job16, int16_t>(k, n, last);
}
static cordic_demod_job job32(size_t k, uint64_t n, bool last = true)
{
	return job_at<cordic_demod_job, int32_t>(k, n, last);
}

// the tiles and tails of `jobs` cover every job exactly, in order: ES bytes per
// sample, 4 * ES per vector
template <typename Job>
static void check_cut(const std::vector<Job> &jobs, int passes, uint64_t ES)
{
	const uint32_t tv = fmd_bank_tile_vecs(passes);
	std::vector<DemodTile> tiles;
	std::vector<DemodTail> tails;
	fmd_bank_cut(jobs.size(), jobs.data(), tv, &tiles, &tails);
	EXPECT(tiles.size() == fmd_bank_count_tiles(jobs.size(), jobs.data(), tv));
	size_t at = 0, tail_at = 0;
	for (const Job &j : jobs) {
		if (j.n == 0)
			continue;
		const uint64_t x = (uintptr_t)j.d_xval, y = (uintptr_t)j.d_yval,
			m = (uintptr_t)j.d_omag, f = (uintptr_t)j.d_ofreq,
			l = (uintptr_t)j.d_last;
		const uint64_t nvec = j.n / 4;
		for (uint64_t v0 = 0; v0 < nvec; v0 += tv) {
			EXPECT(at < tiles.size());
			if (at >= tiles.size())
				return;
			const DemodTile &t = tiles[at++];
			const uint64_t off = v0 * 4 * ES;	// 16 or 8 bytes per vector
			EXPECT(t.x == x + off && t.y == y + off);
			EXPECT(t.mag == m + off && t.freq == f + off);
			EXPECT(t.nvec == (nvec - v0 < tv ? nvec - v0 : tv) && t.nvec >= 1);
			EXPECT(t.first == (v0 ? 0u : 1u) && t.pad == 0);
			EXPECT(t.last == (v0 ? 0 : l));
			EXPECT(t.phase0 == (v0 ? 0u : j.phase0));
			// the halo, one vector in front, lies inside the job
			EXPECT(v0 == 0 || t.x - 4 * ES >= x);
		}
		if (nvec * 4 == j.n && !l)
			continue;
		EXPECT(tail_at < tails.size());
		if (tail_at >= tails.size())
			return;
		const DemodTail &t = tails[tail_at++];
		const uint64_t s0 = nvec ? nvec * 4 - 1 : 0, off = s0 * ES;	// 4 or 2 per sample
		EXPECT(t.x == x + off && t.y == y + off && t.mag == m + off && t.freq == f + off);
		EXPECT(t.last == l && t.phase0 == j.phase0 && t.pad == 0);
		EXPECT(t.count == j.n - s0 && t.count >= 1 && t.count <= 4);
		EXPECT(t.first == (nvec ? 0u : 1u));
		// nothing behind the job's end
		EXPECT(t.x + t.count * ES == x + j.n * ES);
	}
	EXPECT(at == tiles.size() && tail_at == tails.size());
}

int main()
{
	static_assert(sizeof(cordic_demod_job16) == 56 && sizeof(cordic_demod_job) == 56, "");
	const uint64_t lens[] = {0, 1, 3, 4, 5, 7, 8, 1019, 1020, 1021, 1024, 1025, 2043, 2044,
		2045, 4091, 4092, 4093, 4097, 8187, 8188, 8189, 8193, 16379, 40943, 0, 6};
	std::vector<cordic_demod_job16> j16;
	std::vector<cordic_demod_job> j32;
	size_t k = 0;
	for (uint64_t n : lens) {
		j16.push_back(job16(k, n, k % 2 == 0));
		j32.push_back(job32(k, n, k % 2 == 0));
		k++;
	}
	EXPECT(fmd_bank_jobs_valid(j16.size(), j16.data()));
	EXPECT(fmd_bank_jobs_valid(j32.size(), j32.data()));
	for (int p : {1, 2, 4, 8}) {
		check_cut(j16, p, 2);
		check_cut(j32, p, 4);
		// the same table but for the addresses' scale
		EXPECT(fmd_bank_count_tiles(j16.size(), j16.data(), fmd_bank_tile_vecs(p))
			== fmd_bank_count_tiles(j32.size(), j32.data(), fmd_bank_tile_vecs(p)));
	}
	{	// two tiles of one 16-bit job are 8 bytes per vector apart, the 32-bit job's 16
		std::vector<DemodTile> t16, t32;
		std::vector<DemodTail> l16, l32;
		const cordic_demod_job16 a = job16(0, 2 * 1020 + 7);
		const cordic_demod_job b = job32(0, 2 * 1020 + 7);
		fmd_bank_cut(1, &a, 255, &t16, &l16);
		fmd_bank_cut(1, &b, 255, &t32, &l32);
		EXPECT(t16.size() == 3 && t32.size() == 3 && l16.size() == 1 && l32.size() == 1);
		EXPECT(t16[1].x - t16[0].x == 255 * 8 && t32[1].x - t32[0].x == 255 * 16);
		EXPECT(t16[1].freq - t16[0].freq == 255 * 8 && t32[1].freq - t32[0].freq == 255 * 16);
		EXPECT(l16[0].x - t16[0].x == 2043 * 2 && l32[0].x - t32[0].x == 2043 * 4);
		EXPECT(l16[0].count == 4 && l32[0].count == 4);
	}

	// the rules, at one-short granularity
	const uint64_t n = 100;
	const cordic_demod_job16 a = job16(0, n), b = job16(1, n);
	auto valid2 = [](auto p, auto q) {
		const decltype(p) two[2] = {p, q};
		return fmd_bank_jobs_valid(2, two);
	};
	auto one = [](auto p) { return fmd_bank_jobs_valid(1, &p); };
	EXPECT(valid2(a, b));
	// an output over another output by ONE SHORT; adjacent is accepted
	{ cordic_demod_job16 c = b; c.d_omag = a.d_omag + n - 1; EXPECT(!valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_omag = a.d_omag + n; EXPECT(valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_ofreq = a.d_omag - n + 1; EXPECT(!valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_ofreq = a.d_omag - n; EXPECT(valid2(a, c)); }
	{ cordic_demod_job16 c = a; c.d_ofreq = c.d_omag + n - 1; EXPECT(!one(c)); }
	{ cordic_demod_job16 c = a; c.d_ofreq = c.d_omag + n; EXPECT(one(c)); }
	// an output over an input by one short, of the same job and of another
	{ cordic_demod_job16 c = b; c.d_omag = (int16_t *)a.d_xval + n - 1; EXPECT(!valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_omag = (int16_t *)a.d_xval + n; EXPECT(valid2(a, c)); }
	{ cordic_demod_job16 c = a; c.d_ofreq = (int16_t *)c.d_yval + n - 1; EXPECT(!one(c)); }
	// ... where a 32-bit job of the same n would still reach: n * 2 bytes, not n * 4
	{ cordic_demod_job16 c = b; c.d_omag = (int16_t *)a.d_xval + 2 * n - 1; EXPECT(valid2(a, c)); }
	// inputs may alias
	{ cordic_demod_job16 c = b; c.d_xval = a.d_xval; c.d_yval = a.d_xval; EXPECT(valid2(a, c)); }
	// d_last: shared, inside an output, inside an input; next to one is fine
	{ cordic_demod_job16 c = b; c.d_last = a.d_last; EXPECT(!valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_last = (uint32_t *)(a.d_omag + n - 2); EXPECT(!valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_last = (uint32_t *)(a.d_omag + n); EXPECT(valid2(a, c)); }
	{ cordic_demod_job16 c = b; c.d_last = (uint32_t *)(a.d_xval + 2); EXPECT(!valid2(a, c)); }
	// 2-byte alignment is accepted for all four arrays, odd addresses are refused
	for (int w = 0; w < 4; w++)
		for (uintptr_t d = 1; d <= 7; d++) {
			cordic_demod_job16 c = a;
			const int16_t **in = w == 0 ? &c.d_xval : &c.d_yval;
			int16_t **out = w == 2 ? &c.d_omag : &c.d_ofreq;
			if (w < 2)
				*in = (const int16_t *)((uintptr_t)*in + d);
			else
				*out = (int16_t *)((uintptr_t)*out + d);
			EXPECT(one(c) == (d % 2 == 0));
		}
	// d_last stays on the 4-byte grid
	{ cordic_demod_job16 c = a; c.d_last = (uint32_t *)((uintptr_t)c.d_last + 2); EXPECT(!one(c)); }
	{ cordic_demod_job16 c = a; c.d_last = (uint32_t *)((uintptr_t)c.d_last + 4); EXPECT(one(c)); }
	{ cordic_demod_job16 c = a; c.d_xval = nullptr; EXPECT(!one(c)); }
	{ cordic_demod_job16 c = a; c.d_ofreq = nullptr; EXPECT(!one(c)); }
	{ cordic_demod_job16 c = a; c.reserved = 1; EXPECT(!one(c)); }
	{ cordic_demod_job16 c = a; c.n = (~(size_t)0 >> 4) + 1; EXPECT(!one(c)); }
	// a zero-length job's fields are not looked at
	{ cordic_demod_job16 c = a; c.n = 0; c.d_xval = nullptr; c.reserved = 9;
	  c.d_omag = (int16_t *)1; c.d_last = b.d_last; EXPECT(valid2(c, b)); }

	// the 32-bit job type answers as before: the 4-byte grid, n * 4 bytes
	const cordic_demod_job p = job32(0, n), q = job32(1, n);
	EXPECT(valid2(p, q));
	{ cordic_demod_job c = q; c.d_omag = p.d_omag + n - 1; EXPECT(!valid2(p, c)); }
	{ cordic_demod_job c = q; c.d_omag = p.d_omag + n; EXPECT(valid2(p, c)); }
	{ cordic_demod_job c = q; c.d_omag = (int32_t *)p.d_xval + n - 1; EXPECT(!valid2(p, c)); }
	{ cordic_demod_job c = q; c.d_omag = (int32_t *)((uintptr_t)p.d_xval + 2 * n);
	  EXPECT(!valid2(p, c)); }			// inside n * 4, behind n * 2
	{ cordic_demod_job c = p; c.d_xval = (const int32_t *)((uintptr_t)c.d_xval + 2);
	  EXPECT(!one(c)); }				// off the 4-byte grid
	{ cordic_demod_job c = q; c.d_last = p.d_last; EXPECT(!valid2(p, c)); }
	{	// and cuts as before: 16 bytes per vector, 4 per sample
		std::vector<DemodTile> tiles;
		std::vector<DemodTail> tails;
		const cordic_demod_job c = job32(2, 1024 + 2, false);
		fmd_bank_cut(1, &c, 255, &tiles, &tails);
		EXPECT(tiles.size() == 2 && tails.size() == 1);
		EXPECT(tiles[1].x == (uintptr_t)c.d_xval + 255 * 16 && tiles[1].nvec == 1);
		EXPECT(tails[0].x == (uintptr_t)c.d_xval + 1023 * 4 && tails[0].count == 3);
		EXPECT(fmd_bank_count_tiles(1, &c, 255) == 2);
	}
	EXPECT(fmd_bank_jobs_valid(0, nullptr));
	if (!failures)
		std::printf("cutter16 ok\n");
	return failures ? 1 : 0;
}
"""


def test_the_host_cutter_on_16_bit_jobs_under_address_and_ub_sanitizers(tmp_path):
    src, exe = tmp_path / "cutter16.cpp", tmp_path / "cutter16"
    src.write_text(PROGRAM)
    r = subprocess.run(
        ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "cutter16 ok" in r.stdout


def test_one_implementation_serves_both_job_structs():
    """no second copy of the checks or the cutter, and the cutter touches no
    device"""
    text = open(os.path.join(CSRC, "cordic_fm_demod_bank.h")).read()
    for fn in ("fmd_bank_jobs_valid", "fmd_bank_count_tiles", "fmd_bank_cut"):
        assert len(re.findall(r"\binline\s+\w+\s+%s\s*\(" % fn, text)) == 1, fn
    assert "#include <hip" not in text and "hipMalloc" not in text
