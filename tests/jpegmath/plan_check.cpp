// Stand-alone host program (its own main; `make -C tests/jpegmath plan_check` builds it with -fsanitize=address,undefined; never loaded into Python):
// zr::BuildTexturePlan (zetaray_amd/csrc/zr_tex_plan.h), the library's validation of untrusted texture sources, over damaged coefficient records.  Each
// JPEG file named on the command line (tests/jpegmath/make_corpus.py writes them from the fixture) is packed by zrh_jpeg_pack; the record, and MUTANTS
// damaged copies of it (header fields, coef_begin, coefficients; one in four cut short; as host_check.cpp damages them), is handed to the planner as the
// whole payload, in a heap block of exactly its size, as the JPEG_COEF source of one texture next to a RAW_MIP0 and a BC7 source that name the same bytes.
// Required: no sanitizer report, every undamaged record is planned, every mutant is either refused with a message or planned with tables that stay
// inside the payload.  Prints one summary line; exit 0.
#include "../../zetaray_amd/csrc/zr_tex_plan.h"
#include "../../zetaray_amd/host/zr_scene_io.h"
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t Rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

// 1 planned, 0 refused
static int Plan(const std::vector<uint8_t>& rec, uint32_t w, uint32_t h, uint32_t map)
{
    uint8_t* payload = (uint8_t*)std::malloc(rec.size() ? rec.size() : 1);      // (exactly the record's bytes, so that a read beyond them is seen)
    std::memcpy(payload, rec.data(), rec.size());
    zr_texture_desc d[3]; zr_texture_source s[3];
    std::memset(d, 0, sizeof(d)); std::memset(s, 0, sizeof(s));
    d[0].width = (uint16_t)w; d[0].height = (uint16_t)h; d[0].num_mips = 2; d[0].format = map == 0u ? ZR_TEX_RGBA8_SRGB : ZR_TEX_RG8; s[0].encoding = ZR_TEX_SRC_JPEG_COEF;
    d[1].width = 4; d[1].height = 4; d[1].num_mips = 3; d[1].format = ZR_TEX_RGBA8; s[1].encoding = ZR_TEX_SRC_RAW_MIP0;
    d[2].width = 8; d[2].height = 4; d[2].num_mips = 1; d[2].format = ZR_TEX_RGBA8; s[2].encoding = ZR_TEX_SRC_BC7;
    zr::TexturePlan plan; std::string err;
    const int r = zr::BuildTexturePlan(d, s, 3, rec.size(), 1u << 30, payload, zr::kTexSrcAll, zr::kTexPlanAll, plan, err);
    if (r != ZR_OK && (r != ZR_ERR_INVALID_ARG || err.empty())) { std::fprintf(stderr, "a refusal without a message (code %d)\n", r); std::exit(2); }
    if (r == ZR_OK)
    {   // what the kernels would read lies inside the payload: every block's coefficient run, from the table the planner accepted
        if (plan.jpegTexJobs.size() != 1 || plan.blockJobs.size() != 1 || plan.copies.size() != 1 || plan.levels.size() != 2) { std::fprintf(stderr, "a plan of the wrong shape\n"); std::exit(2); }
        for (const zrjp::BlockJob& j : plan.jpegBlockJobs)
        {
            uint32_t last; std::memcpy(&last, payload + j.coef - 4, 4);      // coef_begin[B]
            if (j.coef > rec.size() || j.coef + 2ull * last > rec.size()) { std::fprintf(stderr, "a job that reads beyond the payload\n"); std::exit(2); }
        }
    }
    std::free(payload);
    return r == ZR_OK;
}

int main(int argc, char** argv)
{
    const long mutants = std::getenv("MUTANTS") ? std::atol(std::getenv("MUTANTS")) : 6000;
    size_t files = 0, planned = 0, refused = 0;
    for (int a = 1; a < argc; a++)
    {
        std::ifstream in(argv[a], std::ios::binary);
        if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const uint32_t map = Rnd() % 3u;
        size_t bytes = 0;
        if (zrh_jpeg_pack(argv[a], file.data(), file.size(), map, nullptr, 0, &bytes) != 0) { std::fprintf(stderr, "%s\n", zrh_scene_io_last_error()); return 2; }
        std::vector<uint8_t> good(bytes);
        if (zrh_jpeg_pack(argv[a], file.data(), file.size(), map, good.data(), good.size(), &bytes) != 0) { std::fprintf(stderr, "%s\n", zrh_scene_io_last_error()); return 2; }
        uint32_t w, h; std::memcpy(&w, good.data() + 16, 4); std::memcpy(&h, good.data() + 20, 4);
        if (!Plan(good, w, h, map)) { std::fprintf(stderr, "%s: an undamaged record was refused\n", argv[a]); return 2; }
        files++;
        for (long k = 0; k < mutants; k++)
        {
            std::vector<uint8_t> rec = good;
            if (Rnd() % 4u == 0) rec.resize(Rnd() % rec.size());
            else for (uint32_t n = 1u + Rnd() % 3u; n; n--)
            {
                const size_t at = (Rnd() & 1u) ? Rnd() % (rec.size() < 640u ? rec.size() : 640u) : Rnd() % rec.size();
                rec[at] = (Rnd() & 1u) ? (uint8_t)(rec[at] ^ (1u << (Rnd() % 8u))) : (uint8_t)Rnd();
            }
            (Plan(rec, w, h, map) ? planned : refused)++;
        }
    }
    std::printf("{\"files\": %zu, \"mutants\": %zu, \"planned\": %zu, \"refused\": %zu}\n", files, planned + refused, planned, refused);
    return 0;
}
