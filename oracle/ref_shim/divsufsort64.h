/* Stand-in for the one declaration the reference's AwFmCreate.c takes from libdivsufsort: the suffix array of `text`
 * (bytes compared as unsigned) into `suffixArray`, 0 on success, negative on failure.  A suffix array is a pure function
 * of the text, so the sort behind it (ref_shim.c: this repository's awfmSuffixSort) gives the reference exactly the
 * input the upstream library would have given it. */
#ifndef AWFM_REF_SHIM_DIVSUFSORT64_H
#define AWFM_REF_SHIM_DIVSUFSORT64_H
#include <stdint.h>

int64_t divsufsort64(const uint8_t *text, int64_t *suffixArray, int64_t length);

#endif
