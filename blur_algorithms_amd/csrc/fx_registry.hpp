// fx_registry.hpp -- the window classes the fused and the two-kernel matrix-core kernels are instantiated for, and the one table of
// their entries.  A class is NKB blocks of 16 window positions; its kernels serve every pad <= 8 (NKB - 2):
//   NKB    3   5   7   9  11  13   15   17   19   21   23
//   pad    8  24  40  56  72  88  104  120  136  152  168
// Each family has one instantiation unit, which the Makefile compiles once per class (-DBLUR_INST_NKB) into build/<family>_conv_<NKB>.o:
//   fx_conv.hip   fx_kernels.hpp, three channels per workgroup, NKB <= 11: FxEntry
//   fw_conv.hip   fw_kernels.hpp, one channel per workgroup, every class: FcEntry (one, two and four channels; two: the Cb/Cr plane
//                 of an NV12 surface) and Fw3Entry (three channels, a subset per launch: one sigma per channel); NKB >= 13 also
//                 FxEntry (whole BGR frames, pad 73 .. 168)
//   ff_conv.hip   ff_kernels.hpp, every class, once per pixel type as well (-DBLUR_INST_T; build/ff_[u16_|f16_|bf16_]conv_<NKB>.o):
//                 FfEntryT<T> for float, uint16_t (also two channels: P016), ff_f16 and ff_bf16
//   mx_conv.hip   mx_kernels.hpp, every class: MxEntry
// This header names no entry type and needs no kernel header: engine.hip includes ff_kernels.hpp well after it.
#pragma once
#include <array>
// the only list of the classes in C++ (the Makefile's CLASSES names the objects after it)
#define BLUR_FX_CLASSES(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23)
namespace blur_amd {
constexpr bool fx_is_class(int nkb)
{
#define BLUR_FX_ITEM(NKB_) || nkb == NKB_
    return false BLUR_FX_CLASSES(BLUR_FX_ITEM);
#undef BLUR_FX_ITEM
}
// The entry of type E for one class.  Declared only: every <E, NKB> is an explicit specialisation in its family's instantiation unit,
// so a translation unit that looks entries up (engine.hip) instantiates no kernel.  Every entry type has every class.
template <class E, int NKB> const E* fx_entry();
template <class E> const auto& fx_entries()
{
#define BLUR_FX_ITEM(NKB_) fx_entry<E, NKB_>(),
    static const std::array list = { BLUR_FX_CLASSES(BLUR_FX_ITEM) };
#undef BLUR_FX_ITEM
    return list;
}
// the entry of the class nkb (nullptr: no such class)
template <class E> const E* find_entry(int nkb)
{
    for (const E* e : fx_entries<E>())
        if (e->nkb == nkb) return e;
    return nullptr;
}
// the entry of the smallest class whose window holds the taps of pad (nullptr: none -- the FFT kernels take over)
template <class E> const E* find_entry_for_pad(int pad)
{
    for (const E* e : fx_entries<E>())
        if (8 * (e->nkb - 2) >= pad) return e;
    return nullptr;
}
}  // namespace blur_amd
