// The libsvm text rule, once: which bytes form a regular token, what value a
// regular number has, and which lines a sampling rate keeps.  Compiled by the
// GPU parser (libsvm_parse.hip) and by the host parser (runtime/libsvm.cpp), so
// both decide alike.  Plain C++: no HIP header is needed to include it.
//
// A number of the grammar has an integer mantissa m < 10^15 < 2^53 and a
// decimal exponent |e| <= 22, so (double)m and 10^|e| are exact and
// d = m * 10^e or m / 10^|e| takes one IEEE rounding: d is the correctly
// rounded double of the text.  (float)d equals the correctly rounded float of
// the text -- what strtof returns -- unless d sits exactly on a float tie (the
// first rounding may have landed on it from either side), below FLT_MIN
// (strtof's subnormals round at another bit) or above FLT_MAX.  Such a number
// is *ambiguous*: it makes its line irregular and the caller falls back to the
// libc parser.  The division must stay IEEE: no fast-math on this header.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LSV_HD __host__ __device__ inline
#else
#define LSV_HD inline
#endif

namespace lsv {

LSV_HD bool is_ws(unsigned char c) { return c == ' ' || c == '\t' || c == '\r'; }
LSV_HD bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }

LSV_HD double pow10_exact(int k) {   // 10^k, 0 <= k <= 22: every entry is an exact double
  const double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                        1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[k];
}

constexpr int kMaxDigits = 15;      // significant digits of a mantissa
constexpr int kMaxExp10 = 22;       // |decimal exponent| after the fraction digits are folded in
constexpr int kMaxIndexDigits = 18;

// The float of mantissa m (< 10^15), decimal exponent e (|e| <= 22) and sign.
// Returns false when the number is ambiguous (see above).
LSV_HD bool number_value(uint64_t m, int e, bool neg, float* out) {
  const double d = e >= 0 ? (double)m * pow10_exact(e) : (double)m / pow10_exact(-e);
  uint64_t bits;
  memcpy(&bits, &d, 8);
  if ((bits & 0x1FFFFFFFull) == 0x10000000ull) return false;       // looks like a float tie
  if (d != 0.0 && d < 1.17549435082228750797e-38) return false;    // below FLT_MIN
  if (d > 3.40282346638528859812e+38) return false;                // above FLT_MAX
  const float f = (float)d;
  *out = neg ? -f : f;                                              // -0 -> -0.0f
  return true;
}

// A number of the grammar at [p, e): [+-]? digits ('.' digits*)? exp? | [+-]? '.' digits exp?,
// exp = [eE][+-]?digits.  Returns the position after it, or -1 when no regular
// number starts at p (or it is ambiguous).  `at(i)` reads byte i.
template <typename At>
LSV_HD long long parse_number(const At& at, long long p, long long e, float* out) {
  bool neg = false;
  if (p < e && (at(p) == '+' || at(p) == '-')) { neg = at(p) == '-'; ++p; }
  uint64_t m = 0;
  int nd = 0, any = 0;
  long long frac = 0;
  while (p < e && is_digit(at(p))) {
    const int c = at(p) - '0';
    if (nd > 0 || c) { m = m * 10 + c; ++nd; }
    any = 1; ++p;
    if (nd > kMaxDigits) return -1;
  }
  if (p < e && at(p) == '.') {
    ++p;
    long long fd = 0;
    while (p < e && is_digit(at(p))) {
      const int c = at(p) - '0';
      if (nd > 0 || c) { m = m * 10 + c; ++nd; }
      ++fd; ++p;
      if (nd > kMaxDigits) return -1;
    }
    if (!any && !fd) return -1;       // "." alone
    any = 1;
    frac = fd;
  }
  if (!any) return -1;
  long long ex = 0;   // (saturates far above any exponent the fraction digits could fold back)
  if (p < e && (at(p) == 'e' || at(p) == 'E')) {
    ++p;
    bool eneg = false;
    if (p < e && (at(p) == '+' || at(p) == '-')) { eneg = at(p) == '-'; ++p; }
    if (!(p < e && is_digit(at(p)))) return -1;       // "1e", "1e+"
    while (p < e && is_digit(at(p))) {
      if (ex < 1000000000000000ll) ex = ex * 10 + (at(p) - '0');
      ++p;
    }
    if (eneg) ex = -ex;
  }
  const long long e10 = ex - frac;
  if (e10 > kMaxExp10 || e10 < -kMaxExp10) return -1;
  if (!number_value(m, (int)e10, neg, out)) return -1;
  return p;
}

// One whitespace-delimited token [p, e) of a regular line.  kind: 0 label (a
// number), 1 entry (index ':' number).  Returns false when the token is neither.
template <typename At>
LSV_HD bool parse_token(const At& at, long long p, long long e, int* kind, long long* index, float* value) {
  long long q = p;
  uint64_t idx = 0;
  int nd = 0;
  while (q < e && is_digit(at(q)) && nd <= kMaxIndexDigits) { idx = idx * 10 + (at(q) - '0'); ++q; ++nd; }
  if (q < e && at(q) == ':') {
    if (nd < 1 || nd > kMaxIndexDigits) return false;
    *kind = 1;
    *index = (long long)idx;
    return parse_number(at, q + 1, e, value) == e;
  }
  *kind = 0;
  return parse_number(at, p, e, value) == e;
}

// Sampling: line `ordinal` (a running count of '\n'-separated pieces) is kept
// iff the splitmix64 finaliser of seed ^ ordinal * golden, top 32 bits, is
// below rate * 2^32.  rate >= 1 keeps every line.
LSV_HD bool keep(uint64_t seed, uint64_t ordinal, double rate) {
  if (rate >= 1.0) return true;
  uint64_t z = seed ^ (ordinal * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (z >> 32) < (uint64_t)(rate * 4294967296.0);
}

}  // namespace lsv
