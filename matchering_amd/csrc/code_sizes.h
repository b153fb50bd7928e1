// Code sizes of the big kernels, read from this library's own device code object (wave_util.h, "code warming").
// Host only, and nothing here calls HIP:
// libmgx.so -> section .hip_fatbin -> clang offload bundle -> the gfx950 ELF -> .symtab.  Anything unexpected
// (a compressed bundle, a stripped table) leaves the sizes at zero and the kernels do not warm.
#pragma once

#include <dlfcn.h>
#include <elf.h>

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "wave_util.h"      // CODE_KERNELS, CODE_VARIANTS, CODE_VARIANT_*

namespace mgx {

static const char* const CODE_NAMES[CODE_KERNELS] = {"k_analyzeILi", "k_match_curve", "k_conv_prepILi", "k_convILi",
                                                     "k_correction_round", "k_correction_tail", "k_limitILi"};
static bool elf_ok(const std::vector<char>& f, size_t at) {
    return at + sizeof(Elf64_Ehdr) <= f.size() && std::memcmp(f.data() + at, ELFMAG, SELFMAG) == 0 &&
           f[at + EI_CLASS] == ELFCLASS64;
}
// bytes[family][variant]: variant = the first template argument (log2 of the transform; 256 / 1024 blocks of the
// limiter -> 0 / 1), 0 for plain kernels; the smaller size where two instantiations share a variant
static void code_sizes_from_library(int (&bytes)[CODE_KERNELS][CODE_VARIANTS]) {
    for (auto& row : bytes)
        for (int& b : row) b = 0;
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void*>(&code_sizes_from_library), &info) || !info.dli_fname) return;
    std::ifstream in(info.dli_fname, std::ios::binary);
    if (!in) return;
    const std::vector<char> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (!elf_ok(f, 0)) return;
    const Elf64_Ehdr* eh = reinterpret_cast<const Elf64_Ehdr*>(f.data());
    if (eh->e_shoff + (size_t)eh->e_shnum * sizeof(Elf64_Shdr) > f.size() || eh->e_shstrndx >= eh->e_shnum) return;
    const Elf64_Shdr* sh = reinterpret_cast<const Elf64_Shdr*>(f.data() + eh->e_shoff);
    const char* names = f.data() + sh[eh->e_shstrndx].sh_offset;
    size_t fat = 0, fat_size = 0;
    for (int i = 0; i < eh->e_shnum; ++i)
        if (std::strcmp(names + sh[i].sh_name, ".hip_fatbin") == 0) { fat = sh[i].sh_offset; fat_size = sh[i].sh_size; }
    static const char MAGIC[] = "__CLANG_OFFLOAD_BUNDLE__";
    if (!fat || fat + fat_size > f.size() || fat_size < 32 || std::memcmp(f.data() + fat, MAGIC, 24) != 0) return;
    uint64_t entries = 0;
    std::memcpy(&entries, f.data() + fat + 24, 8);
    size_t pos = fat + 32, dev = 0;
    for (uint64_t e = 0; e < entries && pos + 24 <= fat + fat_size; ++e) {
        uint64_t off = 0, size = 0, tsize = 0;
        std::memcpy(&off, f.data() + pos, 8);
        std::memcpy(&size, f.data() + pos + 8, 8);
        std::memcpy(&tsize, f.data() + pos + 16, 8);
        if (pos + 24 + tsize > fat + fat_size) return;
        const std::string triple(f.data() + pos + 24, f.data() + pos + 24 + tsize);
        if (triple.find("gfx950") != std::string::npos && fat + off + size <= f.size()) dev = fat + off;
        pos += 24 + tsize;
    }
    if (!dev || !elf_ok(f, dev)) return;
    const Elf64_Ehdr* de = reinterpret_cast<const Elf64_Ehdr*>(f.data() + dev);
    if (dev + de->e_shoff + (size_t)de->e_shnum * sizeof(Elf64_Shdr) > f.size()) return;
    const Elf64_Shdr* ds = reinterpret_cast<const Elf64_Shdr*>(f.data() + dev + de->e_shoff);
    for (int i = 0; i < de->e_shnum; ++i) {
        if (ds[i].sh_type != SHT_SYMTAB || ds[i].sh_link >= de->e_shnum) continue;
        const char* str = f.data() + dev + ds[ds[i].sh_link].sh_offset;
        const size_t count = ds[i].sh_size / sizeof(Elf64_Sym);
        const Elf64_Sym* sym = reinterpret_cast<const Elf64_Sym*>(f.data() + dev + ds[i].sh_offset);
        for (size_t k = 0; k < count; ++k) {
            if (ELF64_ST_TYPE(sym[k].st_info) != STT_FUNC || sym[k].st_size == 0) continue;
            const char* name = str + sym[k].st_name;
            if (std::strstr(name, "k_conv_delayILi")) {              // the delay-line convolution: CODE_CONV's last variant
                bytes[CODE_CONV][CODE_VARIANT_CONV_DELAY] = (int)sym[k].st_size;
                continue;
            }
            if (std::strstr(name, "k_conv_wide_prepILi")) {          // ... and its filter preparation
                bytes[CODE_CONV_PREP][CODE_VARIANT_CONV_WIDE] = (int)sym[k].st_size;
                continue;
            }
            if (std::strstr(name, "k_conv_wideILi")) {               // N = 4F: the slot no k_conv<L> uses
                bytes[CODE_CONV][CODE_VARIANT_CONV_WIDE] = (int)sym[k].st_size;
                continue;
            }
            for (int c = 0; c < CODE_KERNELS; ++c) {
                const char* hit = std::strstr(name, CODE_NAMES[c]);
                if (!hit) continue;
                int variant = 0;
                const size_t len = std::strlen(CODE_NAMES[c]);
                if (len >= 3 && std::strcmp(CODE_NAMES[c] + len - 3, "ILi") == 0) {      // templated: ...ILi<number>E
                    const int number = std::atoi(hit + len);
                    variant = number == 256 ? 0 : number == 1024 ? 1 : number;
                }
                if (variant < 0 || variant >= CODE_VARIANTS) continue;
                int& slot = bytes[c][variant];
                if (slot == 0 || (int)sym[k].st_size < slot) slot = (int)sym[k].st_size;
            }
        }
    }
}

}  // namespace mgx
