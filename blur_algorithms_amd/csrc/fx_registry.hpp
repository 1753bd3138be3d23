// fx_registry.hpp -- the window classes (NKB blocks of 16 positions) the fused matrix-core kernels are instantiated for, one
// translation unit per class and kernel file.  A kernel serves every pad <= 8 (NKB - 2).
//   three channels   fx_kernels.hpp (three channels per workgroup) for NKB <= 11 (fx_conv_<NKB>.hip), fw_kernels.hpp (one channel
//                    per workgroup) for 13 .. 23 (fw_conv_<NKB>.hip): FxEntry
//   one, four        fw_kernels.hpp for every class (fw_conv_<NKB>.hip): FcEntry
//   three, a subset  fw_kernels.hpp for every class (fw_conv_<NKB>.hip): Fw3Entry (one sigma per channel)
//   float32          ff_kernels.hpp for every class (ff_conv_<NKB>.hip; ff_registry.hpp): FfEntry
#pragma once
#include "fw_kernels.hpp"
#define BLUR_FX_CLASSES(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(17) X(19) X(21) X(23)
namespace blur_amd {
#define BLUR_FX_DECL(NKB_) const FxEntry* fx_entry_##NKB_(); const FcEntry* fc_entry_##NKB_(); const Fw3Entry* fw3_entry_##NKB_();
BLUR_FX_CLASSES(BLUR_FX_DECL)
#undef BLUR_FX_DECL
inline const FxEntry* find_fx_entry(int pad)
{
#define BLUR_FX_ITEM(NKB_) fx_entry_##NKB_(),
    static const FxEntry* const list[] = { BLUR_FX_CLASSES(BLUR_FX_ITEM) };
#undef BLUR_FX_ITEM
    for (const FxEntry* e : list)
        if (8 * (e->nkb - 2) >= pad) return e;
    return nullptr;
}
inline const FcEntry* find_fc_entry(int nkb)
{
#define BLUR_FC_ITEM(NKB_) fc_entry_##NKB_(),
    static const FcEntry* const list[] = { BLUR_FX_CLASSES(BLUR_FC_ITEM) };
#undef BLUR_FC_ITEM
    for (const FcEntry* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
// three channels, a subset per launch (one sigma per channel): fw_kernels.hpp for every class
inline const Fw3Entry* find_fw3_entry(int nkb)
{
#define BLUR_FW3_ITEM(NKB_) fw3_entry_##NKB_(),
    static const Fw3Entry* const list[] = { BLUR_FX_CLASSES(BLUR_FW3_ITEM) };
#undef BLUR_FW3_ITEM
    for (const Fw3Entry* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
}  // namespace blur_amd
