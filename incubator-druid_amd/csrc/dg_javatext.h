// dg_javatext.h — Java's rules for the strings a query carries, as the host applies them: String.compareTo
// over UTF-8 bytes, StringComparators.NumericComparator, and the number parsers behind the filters on numeric
// columns (Longs.tryParse, BigDecimal(String), Floats / Doubles.tryParse). Host only and no HIP include: a plain
// C++ compiler builds it (tests/filter_plan_main.cpp does, under the sanitizers).
#pragma once
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace dg {

// ------------------------------------------------------------------------------------------------
// Java string ordering (String.compareTo = UTF-16 code units; GenericIndexed.STRING_STRATEGY is
// naturalNullsFirst)
// ------------------------------------------------------------------------------------------------
inline void to_utf16(const std::string& s, std::vector<uint16_t>* out) {
  out->clear();
  for (size_t i = 0; i < s.size();) {
    uint32_t c = (uint8_t)s[i];
    int n = c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
    if (n == 2) c &= 0x1F;
    else if (n == 3) c &= 0x0F;
    else if (n == 4) c &= 0x07;
    for (int k = 1; k < n && i + k < s.size(); ++k) c = (c << 6) | ((uint8_t)s[i + k] & 0x3F);
    i += n;
    if (c >= 0x10000) {
      c -= 0x10000;
      out->push_back((uint16_t)(0xD800 + (c >> 10)));
      out->push_back((uint16_t)(0xDC00 + (c & 0x3FF)));
    } else {
      out->push_back((uint16_t)c);
    }
  }
}

inline int java_compare(const std::string& a, const std::string& b) {
  bool ascii = true;
  for (unsigned char ch : a) ascii &= ch < 0x80;
  for (unsigned char ch : b) ascii &= ch < 0x80;
  if (ascii) {
    int c = a.compare(b);
    return (c > 0) - (c < 0);
  }
  std::vector<uint16_t> ua, ub;
  to_utf16(a, &ua);
  to_utf16(b, &ub);
  size_t n = std::min(ua.size(), ub.size());
  for (size_t i = 0; i < n; ++i)
    if (ua[i] != ub[i]) return ua[i] < ub[i] ? -1 : 1;
  return ua.size() == ub.size() ? 0 : (ua.size() < ub.size() ? -1 : 1);
}

// null-aware compare: null < anything
inline int cmp_nullable(bool an, const std::string& a, bool bn, const std::string& b) {
  if (an || bn) return an == bn ? 0 : (an ? -1 : 1);
  return java_compare(a, b);
}

// StringComparators.NumericComparator (query/ordering/StringComparators.java:346-392)
inline bool try_long(const char* s, long long* out) {
  if (!s || !*s) return false;
  const char* p = s;
  if (*p == '-') p++;
  if (!*p) return false;
  for (const char* q = p; *q; ++q)
    if (*q < '0' || *q > '9') return false;
  errno = 0;
  char* end;
  long long v = strtoll(s, &end, 10);
  if (errno || *end) return false;
  *out = v;
  return true;
}

inline bool try_decimal(const char* s, long double* out) {
  if (!s || !*s) return false;
  // BigDecimal grammar: [+-]digits[.digits][(e|E)[+-]digits] or [+-].digits...
  const char* p = s;
  if (*p == '+' || *p == '-') p++;
  bool digits = false;
  while (*p >= '0' && *p <= '9') p++, digits = true;
  if (*p == '.') {
    p++;
    while (*p >= '0' && *p <= '9') p++, digits = true;
  }
  if (!digits) return false;
  if (*p == 'e' || *p == 'E') {
    p++;
    if (*p == '+' || *p == '-') p++;
    if (!(*p >= '0' && *p <= '9')) return false;
    while (*p >= '0' && *p <= '9') p++;
  }
  if (*p) return false;
  *out = strtold(s, nullptr);
  return true;
}

inline int numeric_compare(const char* a, const char* b) {
  if (a == b) return 0;
  if (!a) return -1;
  if (!b) return 1;
  long long la, lb;
  bool ha = try_long(a, &la), hb = try_long(b, &lb);
  if (ha && hb) return (la > lb) - (la < lb);
  long double da = ha ? (long double)la : 0, db = hb ? (long double)lb : 0;
  bool pa = ha || try_decimal(a, &da), pb = hb || try_decimal(b, &db);
  if (pa && pb) return (da > db) - (da < db);
  if (!pa && !pb) return java_compare(a, b);
  return pa ? 1 : -1;
}

// ------------------------------------------------------------------------------------------------
// numeric post-filters: Java's parsing of the filter's strings (host side, once per call)
// ------------------------------------------------------------------------------------------------
// java.math.BigDecimal(String) (sign, digits with one optional '.', optional [eE][+-]digits; no
// whitespace): value = (neg ? -1 : 1) * digits * 10^exp, digits without leading zeros
struct Decimal {
  bool neg = false;
  std::string digits;  // "" = zero
  long long exp = 0;
};

inline bool parse_big_decimal(const char* s, Decimal* d) {
  if (!s || !*s) return false;
  const char* p = s;
  d->neg = false;
  if (*p == '+' || *p == '-') d->neg = *p++ == '-';
  std::string all;
  long long frac = 0;
  bool dot = false, any = false;
  for (; *p; ++p) {
    if (*p >= '0' && *p <= '9') {
      all.push_back(*p);
      any = true;
      if (dot) frac++;
    } else if (*p == '.' && !dot) {
      dot = true;
    } else {
      break;
    }
  }
  if (!any) return false;
  long long e = 0;
  if (*p == 'e' || *p == 'E') {
    p++;
    bool eneg = false;
    if (*p == '+' || *p == '-') eneg = *p++ == '-';
    if (!(*p >= '0' && *p <= '9')) return false;
    for (; *p >= '0' && *p <= '9'; ++p) {
      e = e * 10 + (*p - '0');
      if (e > 1000000000ll) return false;  // BigDecimal: the exponent must fit an int
    }
    if (eneg) e = -e;
  }
  if (*p) return false;
  size_t z = 0;
  while (z < all.size() && all[z] == '0') z++;
  d->digits = all.substr(z);
  d->exp = e - frac;
  if (d->digits.empty()) d->neg = false;
  return true;
}

// setScale(0, FLOOR / CEILING) (or exact: integral only) then longValueExact. Returns 1 = fits
// *out, 0 = not integral (exact mode), +2 / -2 = beyond Long.MAX / Long.MIN
inline int decimal_to_long(const Decimal& d, int mode /* 0 exact, 1 floor, 2 ceiling */, long long* out) {
  std::string ip;  // integer part digits
  bool frac_nonzero = false;
  if (d.exp >= 0) {
    if (!d.digits.empty()) {
      if (d.digits.size() + (size_t)d.exp > 40) return d.neg ? -2 : 2;
      ip = d.digits + std::string((size_t)d.exp, '0');
    }
  } else {
    const long long k = -d.exp;
    if ((long long)d.digits.size() > k) ip = d.digits.substr(0, d.digits.size() - (size_t)k);
    const std::string fr = (long long)d.digits.size() > k ? d.digits.substr(d.digits.size() - (size_t)k) : d.digits;
    for (char c : fr) frac_nonzero |= c != '0';
  }
  if (mode == 0 && frac_nonzero) return 0;
  if (ip.size() > 20) return d.neg ? -2 : 2;
  unsigned __int128 m = 0;
  for (char c : ip) m = m * 10 + (unsigned)(c - '0');
  __int128 v = d.neg ? -(__int128)m : (__int128)m;
  if (frac_nonzero) {
    if (mode == 1 && d.neg) v -= 1;   // floor of a negative non-integer
    if (mode == 2 && !d.neg) v += 1;  // ceiling of a positive non-integer
  }
  if (v > (__int128)INT64_MAX) return 2;
  if (v < (__int128)INT64_MIN) return -2;
  *out = (long long)v;
  return 1;
}

// GuavaUtils.tryParseLong (a leading '+' stripped) -> Longs.tryParse: [-]digits within range
inline bool guava_try_parse_long(const char* s, long long* out) {
  if (!s || !*s) return false;
  if (*s == '+') s++;
  return try_long(s, out);
}

// DimensionHandlerUtils.getExactLongFromDecimalString (DimensionHandlerUtils.java:404-426)
inline bool exact_long(const char* s, long long* out) {
  if (guava_try_parse_long(s, out)) return true;
  Decimal d;
  if (!parse_big_decimal(s, &d)) return false;
  return decimal_to_long(d, 0, out) == 1;
}

// Guava Floats/Doubles.tryParse: [+-]?(NaN|Infinity|decimal[eE..]?[fFdD]?|0[xX]hex[pP]exp[fFdD]?)
// validated like FLOATING_POINT_PATTERN, then Float.parseFloat / Double.parseDouble (correctly rounded)
inline bool guava_float_syntax(const char* s, std::string* body) {
  if (!s || !*s) return false;
  const char* p = s;
  std::string out;
  if (*p == '+' || *p == '-') out.push_back(*p++);
  if (!strcmp(p, "NaN") || !strcmp(p, "Infinity")) {
    *body = out + p;
    return true;
  }
  auto isx = [](char c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); };
  const char* q = p;
  if (q[0] == '0' && (q[1] == 'x' || q[1] == 'X')) {
    q += 2;
    bool any = false;
    while (isx(*q)) q++, any = true;
    if (*q == '.') {
      q++;
      while (isx(*q)) q++, any = true;
    }
    if (!any || (*q != 'p' && *q != 'P')) return false;
    q++;
    if (*q == '+' || *q == '-') q++;
    if (!(*q >= '0' && *q <= '9')) return false;
    while (*q >= '0' && *q <= '9') q++;
  } else {
    bool any = false;
    while (*q >= '0' && *q <= '9') q++, any = true;
    if (*q == '.') {
      q++;
      while (*q >= '0' && *q <= '9') q++, any = true;
    }
    if (!any) return false;
    if (*q == 'e' || *q == 'E') {
      q++;
      if (*q == '+' || *q == '-') q++;
      if (!(*q >= '0' && *q <= '9')) return false;
      while (*q >= '0' && *q <= '9') q++;
    }
  }
  out.append(p, q);
  if (*q == 'f' || *q == 'F' || *q == 'd' || *q == 'D') q++;
  if (*q) return false;
  *body = out;
  return true;
}

inline bool guava_try_parse_double(const char* s, double* out) {
  std::string b;
  if (!guava_float_syntax(s, &b)) return false;
  *out = strtod(b.c_str(), nullptr);
  return true;
}

inline bool guava_try_parse_float(const char* s, float* out) {
  std::string b;
  if (!guava_float_syntax(s, &b)) return false;
  *out = strtof(b.c_str(), nullptr);
  return true;
}

}  // namespace dg
