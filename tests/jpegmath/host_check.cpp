// Stand-alone host program (its own main; `make -C tests/jpegmath host_check` builds it with -fsanitize=address,undefined; never loaded into Python):
// zrh_jpeg_decode, zrh_jpeg_pack and zrh_jpeg_expand over the valid JPEG files named on the command line (tests/jpegmath/make_corpus.py writes them from
// the fixture), into buffers of exactly the size the sizing call reports, and over MUTANTS random bit flips, byte flips and truncations of each.  Three
// mutants in four keep the headers intact (the damage goes behind the first SOS marker), so that it reaches the Huffman decoder, the restart handling
// and, through the coefficients, the header's arithmetic.  A packed record is also damaged itself and handed to zrh_jpeg_expand, whose check
// (zrjp::CheckRecord) is what the device path relies on.
// Required: no sanitizer report, every valid file decodes, decode and pack agree on what they refuse, every mutant is either refused -- by a message that
// names the file -- or decoded within its buffers.  Prints one summary line; exit 0.
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
static size_t g_records = 0, g_recordsRefused = 0;

[[noreturn]] static void Die(const char* what) { std::fprintf(stderr, "%s: %s\n", what, zrh_scene_io_last_error()); std::exit(2); }

// a record in a heap block of exactly its size -> texels in a block of exactly theirs; 1 expanded, 0 refused
static int Expand(const std::vector<uint8_t>& rec)
{
    uint8_t* in = (uint8_t*)std::malloc(rec.size() ? rec.size() : 1);
    std::memcpy(in, rec.data(), rec.size());
    uint32_t w = 0, h = 0;
    int ok = zrh_jpeg_expand(in, rec.size(), &w, &h, nullptr, 0) == 0;
    if (ok)
    {
        uint32_t map; std::memcpy(&map, in + 28, 4);
        const size_t bytes = (size_t)w * h * (map == 0u ? 4u : 2u);
        uint8_t* out = (uint8_t*)std::malloc(bytes);
        if (zrh_jpeg_expand(in, rec.size(), &w, &h, out, bytes) != 0) Die("the second expansion of the same record failed");
        std::free(out);
    }
    std::free(in);
    return ok;
}
// decodes and packs into buffers of exactly the size the first call reports; 1 decoded, 0 refused
static int Decode(const std::vector<uint8_t>& f, bool mutateRecord)
{
    uint8_t* in = (uint8_t*)std::malloc(f.size() ? f.size() : 1);      // (exactly the file's bytes, so that a read beyond them is seen)
    std::memcpy(in, f.data(), f.size());
    uint32_t w = 0, h = 0;
    int ok = zrh_jpeg_decode("mutant.jpg", in, f.size(), &w, &h, nullptr, 0) == 0;
    if (!ok && !std::strstr(zrh_scene_io_last_error(), "mutant.jpg")) Die("a refusal that does not name the file");
    size_t recBytes = 0;
    const uint32_t map = Rnd() % 3u;
    const int packed = zrh_jpeg_pack("mutant.jpg", in, f.size(), map, nullptr, 0, &recBytes) == 0;
    if (packed != ok) Die("zrh_jpeg_decode and zrh_jpeg_pack disagree on a file");
    if (ok)
    {
        const size_t bytes = (size_t)w * h * 4u;
        uint8_t* out = (uint8_t*)std::malloc(bytes);
        if (zrh_jpeg_decode("mutant.jpg", in, f.size(), &w, &h, out, bytes) != 0) Die("the second decode of the same bytes failed");
        std::free(out);
        std::vector<uint8_t> rec(recBytes);
        if (zrh_jpeg_pack("mutant.jpg", in, f.size(), map, rec.data(), rec.size(), &recBytes) != 0) Die("the second pack of the same bytes failed");
        if (!Expand(rec)) Die("a record the packer wrote was refused");
        if (mutateRecord)
        {   // the record itself, damaged: header fields, coef_begin, coefficients; or cut
            if (Rnd() % 4u == 0) rec.resize(Rnd() % rec.size());
            else for (uint32_t n = 1u + Rnd() % 3u; n; n--)
            {
                const size_t at = (Rnd() & 1u) ? Rnd() % (rec.size() < 640u ? rec.size() : 640u) : Rnd() % rec.size();
                rec[at] = (Rnd() & 1u) ? (uint8_t)(rec[at] ^ (1u << (Rnd() % 8u))) : (uint8_t)Rnd();
            }
            g_records++;
            if (!Expand(rec)) g_recordsRefused++;
        }
    }
    std::free(in);
    return ok;
}

int main(int argc, char** argv)
{
    const long mutants = std::getenv("MUTANTS") ? std::atol(std::getenv("MUTANTS")) : 6000;
    size_t files = 0, decoded = 0, refused = 0;
    for (int a = 1; a < argc; a++)
    {
        std::ifstream in(argv[a], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> good((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (!Decode(good, false)) { std::fprintf(stderr, "%s: a valid file was refused: %s\n", argv[a], zrh_scene_io_last_error()); return 2; }
        files++;
        size_t scan = 0;
        for (size_t i = 0; i + 1 < good.size(); i++) if (good[i] == 0xff && good[i + 1] == 0xda) { scan = i + 2; break; }
        for (long k = 0; k < mutants; k++)
        {
            std::vector<uint8_t> f = good;
            const uint32_t what = Rnd() % 8u;
            if (what == 0) f.resize(Rnd() % f.size());                                                   // truncation
            else if (what == 1) { f.resize(scan + Rnd() % (f.size() - scan)); if (Rnd() & 1u) f[Rnd() % f.size()] ^= (uint8_t)(1u << (Rnd() % 8u)); }
            else for (uint32_t n = 1u + Rnd() % 4u; n; n--)                                              // 1 .. 4 flips: a bit, or a whole byte
            {
                const size_t at = (Rnd() % 4u) ? scan + Rnd() % (f.size() - scan) : Rnd() % f.size();
                f[at] = (Rnd() & 1u) ? (uint8_t)(f[at] ^ (1u << (Rnd() % 8u))) : (uint8_t)Rnd();
            }
            (Decode(f, (k & 3) == 0) ? decoded : refused)++;
        }
    }
    std::printf("{\"files\": %zu, \"mutants\": %zu, \"decoded\": %zu, \"refused\": %zu, \"records\": %zu, \"records_refused\": %zu}\n", files, decoded + refused, decoded, refused,
                g_records, g_recordsRefused);
    return 0;
}
