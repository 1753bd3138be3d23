// ff_registry.hpp -- the fused kernels for float32, u16, float16 and bfloat16 images, one translation unit per pixel type and window
// class of fx_registry.hpp (ff_conv_<NKB>.hip, ff_u16_conv_<NKB>.hip, ff_f16_conv_<NKB>.hip, ff_bf16_conv_<NKB>.hip).  A kernel serves every pad <= 8 (NKB - 2).
#pragma once
#include "ff_kernels.hpp"
#include "fx_registry.hpp"
namespace blur_amd {
#define BLUR_FF_DECL(NKB_) const FfEntry* ff_entry_##NKB_();
BLUR_FX_CLASSES(BLUR_FF_DECL)
#undef BLUR_FF_DECL
inline const FfEntry* find_ff_entry(int nkb)
{
#define BLUR_FF_ITEM(NKB_) ff_entry_##NKB_(),
    static const FfEntry* const list[] = { BLUR_FX_CLASSES(BLUR_FF_ITEM) };
#undef BLUR_FF_ITEM
    for (const FfEntry* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
#define BLUR_FF_DECL(NKB_) const FfEntryU16* ff_u16_entry_##NKB_();
BLUR_FX_CLASSES(BLUR_FF_DECL)
#undef BLUR_FF_DECL
inline const FfEntryU16* find_ff_u16_entry(int nkb)
{
#define BLUR_FF_ITEM(NKB_) ff_u16_entry_##NKB_(),
    static const FfEntryU16* const list[] = { BLUR_FX_CLASSES(BLUR_FF_ITEM) };
#undef BLUR_FF_ITEM
    for (const FfEntryU16* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
#define BLUR_FF_DECL(NKB_) const FfEntryF16* ff_f16_entry_##NKB_();
BLUR_FX_CLASSES(BLUR_FF_DECL)
#undef BLUR_FF_DECL
inline const FfEntryF16* find_ff_f16_entry(int nkb)
{
#define BLUR_FF_ITEM(NKB_) ff_f16_entry_##NKB_(),
    static const FfEntryF16* const list[] = { BLUR_FX_CLASSES(BLUR_FF_ITEM) };
#undef BLUR_FF_ITEM
    for (const FfEntryF16* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
#define BLUR_FF_DECL(NKB_) const FfEntryBf16* ff_bf16_entry_##NKB_();
BLUR_FX_CLASSES(BLUR_FF_DECL)
#undef BLUR_FF_DECL
inline const FfEntryBf16* find_ff_bf16_entry(int nkb)
{
#define BLUR_FF_ITEM(NKB_) ff_bf16_entry_##NKB_(),
    static const FfEntryBf16* const list[] = { BLUR_FX_CLASSES(BLUR_FF_ITEM) };
#undef BLUR_FF_ITEM
    for (const FfEntryBf16* e : list)
        if (e->nkb == nkb) return e;
    return nullptr;
}
}  // namespace blur_amd
