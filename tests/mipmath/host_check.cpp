// Stand-alone host program (its own main; `make -C tests/mipmath host_check` builds it with -fsanitize=address,undefined; never loaded into Python):
//   1. include/zr_mipgen.h through zrh_mip_generate, every size 1 x 1 .. 9 x 7 in the three formats, into heap buffers of exactly the chain's size
//   2. zrh_png_decode over the valid PNG files named on the command line (tests/mipmath/make_corpus.py writes them), into exact-size buffers, and over
//      MUTANTS random byte flips and truncations of each.  Half of the mutants get the CRC of every chunk mended, so that the damage reaches the
//      inflate, filter and conversion code instead of stopping at the first CRC.
// Required: no sanitizer report, every valid file decodes, every mutant is either refused or decoded.  Prints one summary line; exit 0.
#include "../../zetaray_amd/host/zr_scene_io.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t Rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

static uint32_t Crc(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1; }
    return c ^ 0xffffffffu;
}
// rewrites the CRC of every chunk that lies whole inside the file
static void MendCrcs(std::vector<uint8_t>& f)
{
    for (size_t at = 8; f.size() >= 12 && at <= f.size() - 12;)
    {
        const size_t len = ((size_t)f[at] << 24) | ((size_t)f[at + 1] << 16) | ((size_t)f[at + 2] << 8) | f[at + 3];
        if (len > f.size() - at - 12) break;
        const uint32_t c = Crc(f.data() + at + 4, 4 + len);
        uint8_t* q = f.data() + at + 8 + len;
        q[0] = (uint8_t)(c >> 24); q[1] = (uint8_t)(c >> 16); q[2] = (uint8_t)(c >> 8); q[3] = (uint8_t)c;
        at += 12 + len;
    }
}
// decodes into a buffer of exactly the size the first call reports; 1 decoded, 0 refused
static int Decode(const std::vector<uint8_t>& f)
{
    // (the file's bytes in a heap block of exactly their number, so that a read beyond them is seen)
    uint8_t* in = (uint8_t*)std::malloc(f.size() ? f.size() : 1);
    std::memcpy(in, f.data(), f.size());
    uint32_t w = 0, h = 0;
    int ok = zrh_png_decode("mutant.png", in, f.size(), &w, &h, nullptr, 0) == 0;
    if (ok)
    {
        const size_t bytes = (size_t)w * h * 4u;
        uint8_t* out = (uint8_t*)std::malloc(bytes);
        ok = zrh_png_decode("mutant.png", in, f.size(), &w, &h, out, bytes) == 0;
        if (!ok) { std::fprintf(stderr, "the second decode of the same bytes failed: %s\n", zrh_scene_io_last_error()); std::exit(2); }
        std::free(out);
    }
    else if (!std::strstr(zrh_scene_io_last_error(), "mutant.png")) { std::fprintf(stderr, "a refusal that does not name the file: %s\n", zrh_scene_io_last_error()); std::exit(2); }
    std::free(in);
    return ok;
}

int main(int argc, char** argv)
{
    // ---- 1. the header
    size_t chains = 0;
    for (uint32_t fmt = 0; fmt <= ZR_TEX_RG8; fmt++) for (uint32_t w = 1; w <= 9; w++) for (uint32_t h = 1; h <= 7; h++)
    {
        zr_texture_desc d; std::memset(&d, 0, sizeof(d));
        d.width = (uint16_t)w; d.height = (uint16_t)h; d.format = (uint8_t)fmt; d.num_mips = 1;
        for (uint32_t m = w > h ? w : h; m > 1; m >>= 1) d.num_mips++;
        const uint32_t bpp = fmt == ZR_TEX_RG8 ? 2u : 4u;
        size_t bytes = 0;
        for (uint32_t m = 0; m < d.num_mips; m++) bytes += (size_t)((w >> m) ? (w >> m) : 1u) * ((h >> m) ? (h >> m) : 1u) * bpp;
        uint8_t* heap = (uint8_t*)std::malloc(bytes);
        for (size_t i = 0; i < (size_t)w * h * bpp; i++) heap[i] = (uint8_t)Rnd();
        if (zrh_mip_generate(&d, 1, heap) != 0) { std::fprintf(stderr, "zrh_mip_generate failed: %s\n", zrh_scene_io_last_error()); return 2; }
        volatile uint8_t sink = heap[bytes - 1]; (void)sink;
        std::free(heap);
        chains++;
    }
    // ---- 2. the PNG decoder
    const long mutants = std::getenv("MUTANTS") ? std::atol(std::getenv("MUTANTS")) : 2000;
    size_t files = 0, decoded = 0, refused = 0;
    for (int a = 1; a < argc; a++)
    {
        std::ifstream in(argv[a], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> good((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (!Decode(good)) { std::fprintf(stderr, "%s: a valid file was refused: %s\n", argv[a], zrh_scene_io_last_error()); return 2; }
        files++;
        for (long k = 0; k < mutants; k++)
        {
            std::vector<uint8_t> f = good;
            const uint32_t what = Rnd() % 8u;
            if (what == 0) f.resize(Rnd() % f.size());                                                   // truncation
            else if (what == 1) { f.resize(Rnd() % f.size()); if (!f.empty()) f[Rnd() % f.size()] ^= (uint8_t)(1u << (Rnd() % 8u)); }
            else for (uint32_t n = 1u + Rnd() % 4u; n; n--)                                              // 1 .. 4 flips: a bit, or a whole byte
            {
                const size_t at = (Rnd() % 4u) ? 8u + Rnd() % (f.size() - 8u) : Rnd() % f.size();
                f[at] = (Rnd() & 1u) ? (uint8_t)(f[at] ^ (1u << (Rnd() % 8u))) : (uint8_t)Rnd();
            }
            if (k & 1) MendCrcs(f);
            (Decode(f) ? decoded : refused)++;
        }
    }
    std::printf("{\"chains\": %zu, \"files\": %zu, \"mutants\": %zu, \"decoded\": %zu, \"refused\": %zu}\n", chains, files, decoded + refused, decoded, refused);
    return 0;
}
