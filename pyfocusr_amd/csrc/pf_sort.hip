// The library's one entry to the device radix sort (pf_sort_pairs, declared in pf_internal.h): every unit
// sorts through it, so hipCUB's sort kernels are instantiated here, once per key width.
#include <hipcub/hipcub.hpp>

#include "pf_internal.h"

namespace {

template <class Key>
void sort_pairs(Scratch& sc, const Key* k_in, Key* k_out, const int32_t* v_in, int32_t* v_out, int64_t n, int end_bit) {
    if (n >= ((int64_t)1 << 31)) sc.note(hipErrorInvalidValue);  // the count goes to hipCUB as an int
    size_t need = 0;
    if (sc.ok()) sc.note(hipcub::DeviceRadixSort::SortPairs(nullptr, need, k_in, k_out, v_in, v_out, (int)n, 0, end_bit, sc.st));
    void* tmp = sc.get<char>(need);
    if (sc.ok()) sc.note(hipcub::DeviceRadixSort::SortPairs(tmp, need, k_in, k_out, v_in, v_out, (int)n, 0, end_bit, sc.st));
}

}  // namespace

void pf_sort_pairs(Scratch& sc, const unsigned* k_in, unsigned* k_out, const int32_t* v_in, int32_t* v_out, int64_t n, int end_bit) {
    sort_pairs(sc, k_in, k_out, v_in, v_out, n, end_bit);
}

void pf_sort_pairs(Scratch& sc, const unsigned long long* k_in, unsigned long long* k_out, const int32_t* v_in, int32_t* v_out,
                   int64_t n, int end_bit) {
    sort_pairs(sc, k_in, k_out, v_in, v_out, n, end_bit);
}
