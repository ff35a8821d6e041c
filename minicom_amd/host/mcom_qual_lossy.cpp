// minicom_amd/host/mcom_qual_lossy.cpp -- lossy quality values on the host: the twin of csrc/qual_lossy.hip.
// Plain C++ on host buffers -- no GPU, no HIP call.  The spec text, the maps, the idempotence rule and the P-block walk are those of
// csrc/qual_lossy.hpp, which the kernels compile as well, so the bytes and the report equal the device's and the same specs are
// refused.  Builds alone (tests/fuzz_qual_lossy.cpp runs it under the sanitizers).
#include "../../include/mcom_host.h"
#include "../csrc/qual_lossy.hpp"
#include <cstdio>
#include <cstring>
#include <string>

using namespace mcom_qlossy;

static_assert(sizeof(Spec) == sizeof(mcomh_qual_lossy_spec) && sizeof(Report) == sizeof(mcomh_qual_lossy_report), "qual_lossy.hpp states the layouts of include/mcom_host.h");

extern "C" int mcomh_qual_lossy_parse(const char *text, mcomh_qual_lossy_spec *spec)
{
	if (!text || !spec) return -1;
	Spec s;
	if (!parse(text, s)) return -1;
	memcpy(spec, &s, sizeof s);
	return 0;
}

extern "C" int mcomh_qual_lossy_print(const mcomh_qual_lossy_spec *spec, char *text, size_t cap)
{
	if (!spec || !text) return -1;
	Spec s;
	memcpy(&s, spec, sizeof s);
	return print(s, text, cap) ? 0 : -1;
}

extern "C" int mcomh_qual_transform(uint8_t *rows, uint64_t n_rows, uint32_t L, uint64_t pitch, const mcomh_qual_lossy_spec *spec, mcomh_qual_lossy_report *report)
{
	if (!spec || (n_rows && !rows) || L < 1 || L > 256 || pitch < L || n_rows >= ((uint64_t)1 << 32)) return -1;
	Spec s;
	memcpy(&s, spec, sizeof s);
	uint8_t lut[256];
	if (!resolve(s, lut)) return -1;
	Report r = {0, 0, 0, 0};
	for (uint64_t i = 0; i < n_rows; ++i) {
		uint8_t *q = rows + i * pitch;
		RowStat st;
		if (s.kind == K_PBLOCK) pblock_row(q, L, s.p[0], st);
		else for (uint32_t j = 0; j < L; ++j) { const uint8_t o = lut[q[j]]; st.add(q[j], o); q[j] = o; }
		r.changed += st.changed; r.sum_abs += st.sum_abs; r.sum_sq += st.sum_sq;
		if (st.max_abs > r.max_abs) r.max_abs = st.max_abs;
	}
	if (report) memcpy(report, &r, sizeof r);
	return 0;
}

// FOLDER/qual_lossy.txt: the canonical text of a spec and one newline, nothing else
extern "C" int mcomh_qual_lossy_marker(const char *folder, mcomh_qual_lossy_spec *spec, char *text, size_t cap)
{
	if (!folder || !spec) return -1;
	FILE *f = fopen((std::string(folder) + "/qual_lossy.txt").c_str(), "rb");
	if (!f) return 0;
	char buf[SPEC_TEXT_MAX + 2];
	const size_t got = fread(buf, 1, sizeof buf, f);
	fclose(f);
	if (got < 2 || got > SPEC_TEXT_MAX || buf[got - 1] != '\n' || memchr(buf, 0, got)) return -1;
	buf[got - 1] = 0;
	Spec s;
	if (!parse(buf, s)) return -1;
	if (text) { if (cap < got) return -1; memcpy(text, buf, got); }
	memcpy(spec, &s, sizeof s);
	return 1;
}
