// TEST-ONLY, stand-alone: the glTF loader's skin paths (zetaray_amd/host/zr_scene_io.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU.
// Loads the fixture (tests/golden/skin_gltf laid out in argv[1] by tests/skinmath/cases.py: skinned_gltf) and damaged variants of it -- joint indices,
// accessor counts, skin joint lists and buffer sizes out of range, truncated buffers, flipped bytes.  Every variant must be refused (-1 with a message)
// or load with tables that hold: each loaded scene's skin and animation tables are walked index by index.  Prints the counts; exit status 1 when the
// intact fixture does not load or a loaded variant's tables do not hold.  `make -C tests/skinmath fuzz` builds and runs it.
#include "../../zetaray_amd/host/zr_scene_io.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

static std::vector<char> Read(const std::string& p) { std::ifstream f(p, std::ios::binary); return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>()); }
static void Write(const std::string& p, const char* d, size_t n) { std::ofstream f(p, std::ios::binary | std::ios::trunc); f.write(d, (std::streamsize)n); }

static int g_loaded = 0, g_refused = 0, g_bad = 0;
static const uint16_t kRho[1] = {0};
static const uint32_t kRhoDim[3] = {1, 1, 1};

// the tables of a loaded scene, every index followed
static bool TablesHold(const zrh_scene_data* s)
{
    const zr_scene_desc* d = zrh_scene_data_desc(s);
    const zr_anim_desc* a = zrh_scene_data_animation(s);
    const zr_skin_desc* k = zrh_scene_data_skinning(s);
    volatile double sum = 0;      // (every table entry is read)
    for (uint32_t i = 0; i < d->num_instances; i++)
    {
        const zr_mesh_instance& I = d->instances[i];
        if ((uint64_t)I.base_idx_offset + 3ull * d->instance_num_tris[i] > d->num_indices) return false;
        for (uint32_t t = 0; t < 3 * d->instance_num_tris[i]; t++)
        {
            const uint64_t v = (uint64_t)I.base_vtx_offset + d->indices[I.base_idx_offset + t];
            if (v >= d->num_vertices) return false;
            sum += d->vertices[v].pos[0];
        }
    }
    if (!k) return true;
    if (!a) return false;
    for (uint32_t j = 0; j < k->num_joints; j++) { if (k->joints[j].node >= a->num_nodes) return false; sum += k->joints[j].inverse_bind[11]; }
    for (uint32_t r = 0; r < k->num_ranges; r++)
    {
        const zr_skin_range& g = k->ranges[r];
        if ((uint64_t)g.first_vertex + g.num_vertices > d->num_vertices || (uint64_t)g.first_influence + g.num_vertices > k->num_influences) return false;
        for (uint32_t v = 0; v < g.num_vertices; v++)
            for (int c = 0; c < 4; c++)
            {
                const zr_skin_influence& f = k->influences[g.first_influence + v];
                if (f.joint[c] >= k->num_joints) return false;
                sum += f.weight[c] * k->joints[f.joint[c]].inverse_bind[0] + d->vertices[g.first_vertex + v].pos[1];
            }
    }
    // ... and the host form poses them
    std::vector<zr_vertex> rest, out;
    for (uint32_t r = 0; r < k->num_ranges; r++) rest.insert(rest.end(), d->vertices + k->ranges[r].first_vertex, d->vertices + k->ranges[r].first_vertex + k->ranges[r].num_vertices);
    out.resize(rest.size());
    if (zrh_skin_pose(a, k, 0.6f, rest.data(), out.data())) return false;
    for (const zr_vertex& v : out) sum += v.pos[2];
    return true;
}
static int Try(const std::string& gltf)
{
    zrh_scene_data* s = nullptr;
    if (zrh_gltf_load(gltf.c_str(), kRho, kRhoDim, &s) != 0) { g_refused++; return -1; }
    if (!TablesHold(s)) { g_bad++; std::fprintf(stderr, "tables do not hold: %s\n", gltf.c_str()); }
    g_loaded++;
    zrh_scene_data_destroy(s);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: fuzz_loader DIR (the fixture laid out by tests/skinmath/cases.py: skinned_gltf)\n"); return 2; }
    const std::string dir = argv[1], gltf = dir + "/cornell_skinned.gltf", bin = dir + "/skin_tube.bin", var = dir + "/variant.gltf";
    const std::vector<char> text = Read(gltf), blob = Read(bin);
    if (text.empty() || blob.empty()) { std::fprintf(stderr, "no fixture in %s\n", dir.c_str()); return 2; }
    if (Try(gltf) != 0 || g_bad) { std::fprintf(stderr, "the intact fixture does not load: %s\n", zrh_scene_io_last_error()); return 1; }
    const std::string json(text.begin(), text.end());
    int variants = 0;
    // ---- JSON: every number behind the keys below, one at a time, replaced by values out of range
    const char* keys[] = {"\"count\":", "\"byteLength\":", "\"byteOffset\":", "\"bufferView\":", "\"inverseBindMatrices\":", "\"skin\":", "\"JOINTS_0\":", "\"WEIGHTS_0\":", "\"sampler\":", "\"node\":", "\"mesh\":"};
    const char* values[] = {"0", "1", "7", "99999", "4000000000", "-1"};
    for (const char* key : keys)
        for (size_t at = json.find(key); at != std::string::npos; at = json.find(key, at + 1))
        {
            size_t b = at + std::strlen(key); while (b < json.size() && json[b] == ' ') b++;
            size_t e = b; while (e < json.size() && (std::isdigit((unsigned char)json[e]) || json[e] == '-' || json[e] == '.')) e++;
            if (e == b) continue;
            for (const char* v : values)
            {
                const std::string m = json.substr(0, b) + v + json.substr(e);
                Write(var, m.data(), m.size()); Try(var); variants++;
            }
        }
    // ---- the skin's joint list: each entry out of range, the list shortened and emptied
    {
        const size_t sk = json.find("\"skins\""), jl = json.find("\"joints\":", sk), lb = json.find('[', jl), rb = json.find(']', lb);
        const char* lists[] = {"[]", "[0]", "[99999, 1, 2]", "[-1, -2, -3]", "[12, 13]", "[12, 12, 12, 12, 12, 12, 12, 12]", "[1e30, 0, 0]", "[14, 13, 12]"};
        for (const char* l : lists) { const std::string m = json.substr(0, lb) + l + json.substr(rb + 1); Write(var, m.data(), m.size()); Try(var); variants++; }
    }
    // ---- the tube's buffer: truncated, and bytes overwritten (joint indices and weights among them) with a fixed-seed generator
    for (size_t n = 0; n < blob.size(); n += blob.size() / 48 + 1) { Write(bin, blob.data(), n); Try(gltf); variants++; }
    uint32_t seed = 12345u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (int i = 0; i < 256; i++)
    {
        std::vector<char> m = blob;
        const int flips = 1 + (int)(next() % 64u);
        for (int f = 0; f < flips; f++) m[next() % m.size()] = (char)(i % 3 == 0 ? 0xff : next());
        Write(bin, m.data(), m.size()); Try(gltf); variants++;
    }
    Write(bin, blob.data(), blob.size());
    std::printf("fuzz_loader: %d variants + the intact fixture: %d loaded within bounds, %d refused, %d with tables that do not hold\n", variants, g_loaded, g_refused, g_bad);
    return g_bad ? 1 : 0;
}
