// Prints the ABI facts of the drop-in boundary as one JSON object: the vtable slot of every virtual of
// IAlignment / IConfig / ILog (Itanium ABI), the slot of each destructor, sizes and field offsets of Align,
// AlignmentPosition and ILog, and cCookie.  Built against include/ngm_ialignment.h by default; with
// -DABI_PROBE_REFERENCE against the reference's IAlignment.h / IConfig.h / ILog.h (by -I path) to regenerate
// tests/golden/ialignment_abi.json (oracle/make_abi_golden.py).  A signature the other header set does not
// declare fails to compile.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <set>
#include <type_traits>

#ifdef ABI_PROBE_REFERENCE
#include "IAlignment.h"
#include "IConfig.h"
#include "ILog.h"
ILog const *_log = 0;
IConfig *_config = 0;
#else
#include "ngm_ialignment.h"
#endif

// Itanium C++ ABI: a pointer to a virtual member function holds 1 + the byte offset of its vtable entry
template <class P> static long slot(P p) {
	static_assert(sizeof(P) == 2 * sizeof(std::ptrdiff_t), "Itanium member-function pointer expected");
	std::ptrdiff_t w[2];
	std::memcpy(w, &p, sizeof w);
	return (w[0] & 1) ? (long) ((w[0] - 1) / (std::ptrdiff_t) sizeof(void *)) : -1;
}

static bool first = true;
static void put(char const *key, long v) {
	std::printf("%s\n  \"%s\": %ld", first ? "{" : ",", key, v);
	first = false;
}

// the virtual destructor takes the two entries that no named virtual occupies (complete and deleting)
static long dtor_slot(std::set<long> const &named) {
	for (long s = 0; s < (long) named.size() + 2; ++s)
		if (!named.count(s)) return s;
	return -1;
}

typedef char const *const *const SeqList;

int main() {
	std::set<long> a, c, l;
	long v;
#define SLOT(set, key, expr) v = slot(expr); set.insert(v); put(key, v)
	SLOT(a, "IAlignment::GetScoreBatchSize", static_cast<int (IAlignment::*)() const>(&IAlignment::GetScoreBatchSize));
	SLOT(a, "IAlignment::GetAlignBatchSize", static_cast<int (IAlignment::*)() const>(&IAlignment::GetAlignBatchSize));
	SLOT(a, "IAlignment::BatchScore",
			static_cast<int (IAlignment::*)(int const, int const, SeqList, SeqList, SeqList, float *const, void *)>(&IAlignment::BatchScore));
	SLOT(a, "IAlignment::BatchAlign",
			static_cast<int (IAlignment::*)(int const, int const, SeqList, SeqList, SeqList, Align *const, void *)>(&IAlignment::BatchAlign));
	put("IAlignment::~IAlignment", dtor_slot(a));
	SLOT(c, "IConfig::GetString", static_cast<char const *(IConfig::*)(char const *const) const>(&IConfig::GetString));
	SLOT(c, "IConfig::GetInt(name)", static_cast<int (IConfig::*)(char const *const) const>(&IConfig::GetInt));
	SLOT(c, "IConfig::GetInt(name,min,max)", static_cast<int (IConfig::*)(char const *const, int, int) const>(&IConfig::GetInt));
	SLOT(c, "IConfig::GetParameter", static_cast<int (IConfig::*)(char const *const) const>(&IConfig::GetParameter));
	SLOT(c, "IConfig::GetFloat(name)", static_cast<float (IConfig::*)(char const *const) const>(&IConfig::GetFloat));
	SLOT(c, "IConfig::GetFloat(name,min,max)", static_cast<float (IConfig::*)(char const *const, float, float) const>(&IConfig::GetFloat));
	SLOT(c, "IConfig::GetIntArray", static_cast<int (IConfig::*)(char const *const, int *, int) const>(&IConfig::GetIntArray));
	SLOT(c, "IConfig::GetFloatArray", static_cast<int (IConfig::*)(char const *const, float *, int) const>(&IConfig::GetFloatArray));
	SLOT(c, "IConfig::GetDoubleArray", static_cast<int (IConfig::*)(char const *const, double *, int) const>(&IConfig::GetDoubleArray));
	SLOT(c, "IConfig::Exists", static_cast<bool (IConfig::*)(char const *const) const>(&IConfig::Exists));
	SLOT(c, "IConfig::HasArray", static_cast<bool (IConfig::*)(char const *const) const>(&IConfig::HasArray));
	put("IConfig::~IConfig", dtor_slot(c));
	SLOT(l, "ILog::_Message", static_cast<void (ILog::*)(int const, char const *const, char const *const, ...) const>(&ILog::_Message));
	SLOT(l, "ILog::_Debug", static_cast<void (ILog::*)(int const, char const *const, char const *const, ...) const>(&ILog::_Debug));
	put("ILog::~ILog", dtor_slot(l));
#undef SLOT
	put("virtual_destructors", std::has_virtual_destructor<IAlignment>::value + std::has_virtual_destructor<IConfig>::value +
			std::has_virtual_destructor<ILog>::value);
	put("sizeof(IAlignment)", sizeof(IAlignment));
	put("sizeof(IConfig)", sizeof(IConfig));
	put("sizeof(ILog)", sizeof(ILog));
	put("offsetof(ILog, null)", offsetof(ILog, null));
	put("sizeof(Align)", sizeof(Align));
	put("offsetof(Align, pBuffer1)", offsetof(Align, pBuffer1));
	put("offsetof(Align, pBuffer2)", offsetof(Align, pBuffer2));
	put("offsetof(Align, ExtendedData)", offsetof(Align, ExtendedData));
	put("offsetof(Align, PositionOffset)", offsetof(Align, PositionOffset));
	put("offsetof(Align, QStart)", offsetof(Align, QStart));
	put("offsetof(Align, QEnd)", offsetof(Align, QEnd));
	put("offsetof(Align, Score)", offsetof(Align, Score));
	put("offsetof(Align, Identity)", offsetof(Align, Identity));
	put("offsetof(Align, NM)", offsetof(Align, NM));
	put("sizeof(AlignmentPosition)", sizeof(AlignmentPosition));
	put("offsetof(AlignmentPosition, type)", offsetof(AlignmentPosition, type));
	put("offsetof(AlignmentPosition, readPosition)", offsetof(AlignmentPosition, readPosition));
	put("offsetof(AlignmentPosition, refPosition)", offsetof(AlignmentPosition, refPosition));
	put("offsetof(AlignmentPosition, match)", offsetof(AlignmentPosition, match));
	put("cCookie", cCookie);
	std::printf("\n}\n");
	return 0;
}
