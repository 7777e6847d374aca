// TEST-ONLY, stand-alone: the glTF loader's morph-target paths (zetaray_amd/host/zr_scene_io.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the
// CPU.  Loads the fixture (tests/golden/morph_gltf laid out in argv[1] by tests/morphmath/cases.py: morphed_gltf) and damaged variants of it -- accessor,
// view, target and sampler indices, counts and offsets out of range, sparse counts and sparse indices out of range, truncated buffers, flipped bytes.
// Every variant must be refused (-1 with a message) or load with tables that hold: each loaded scene's morph, skin and animation tables are walked
// index by index and posed by the host form.  Prints the counts; exit status 1 when the intact fixture does not load or a loaded variant's tables do
// not hold.  `make -C tests/morphmath fuzz` builds and runs it.
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
    const zr_morph_desc* m = zrh_scene_data_morph(s);
    if (m)
    {
        if (!a) return false;
        std::vector<zr_vertex> rest, out;
        for (uint32_t r = 0; r < m->num_ranges; r++)
        {
            const zr_morph_range& g = m->ranges[r];
            if ((uint64_t)g.first_vertex + g.num_vertices > d->num_vertices || (uint64_t)g.first_target + g.num_targets > m->num_targets || g.track >= m->num_tracks) return false;
            const zr_morph_track& tr = m->tracks[g.track];
            if (tr.num_targets != g.num_targets || (uint64_t)tr.first_key + tr.num_keys > m->num_times || (uint64_t)tr.first_value + (uint64_t)tr.num_keys * tr.num_targets > m->num_values) return false;
            for (uint32_t k2 = 0; k2 < tr.num_keys; k2++) sum += m->times[tr.first_key + k2];
            for (uint64_t k2 = 0; k2 < (uint64_t)tr.num_keys * tr.num_targets; k2++) sum += m->values[tr.first_value + k2];
            for (uint32_t t = 0; t < g.num_targets; t++)
            {
                const zr_morph_target& tg = m->targets[g.first_target + t];
                for (uint32_t first : {tg.first_pos, tg.first_nrm, tg.first_tan})
                {
                    if (first == ZR_MORPH_NONE) continue;
                    if ((uint64_t)first + g.num_vertices > m->num_deltas) return false;
                    for (uint32_t v = 0; v < g.num_vertices; v++) sum += m->deltas[3 * ((size_t)first + v) + 2];
                }
            }
            rest.insert(rest.end(), d->vertices + g.first_vertex, d->vertices + g.first_vertex + g.num_vertices);
        }
        out.resize(rest.size());
        // ... and the host form poses them (through the skin, where a range has one)
        if (zrh_morph_pose(a, k, m, 0.6f, rest.data(), out.data())) return false;
        for (const zr_vertex& v : out) sum += v.pos[2];
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
    if (argc < 2) { std::fprintf(stderr, "usage: fuzz_loader DIR (the fixture laid out by tests/morphmath/cases.py: morphed_gltf)\n"); return 2; }
    const std::string dir = argv[1], gltf = dir + "/cornell_morphed.gltf", bin = dir + "/morph.bin", var = dir + "/variant.gltf";
    const std::vector<char> text = Read(gltf), blob = Read(bin);
    if (text.empty() || blob.empty()) { std::fprintf(stderr, "no fixture in %s\n", dir.c_str()); return 2; }
    if (Try(gltf) != 0 || g_bad) { std::fprintf(stderr, "the intact fixture does not load: %s\n", zrh_scene_io_last_error()); return 1; }
    const std::string json(text.begin(), text.end());
    int variants = 0;
    // ---- JSON: every number behind the keys below, one at a time, replaced by values out of range
    const char* keys[] = {"\"count\":", "\"byteLength\":", "\"byteOffset\":", "\"byteStride\":", "\"bufferView\":", "\"componentType\":", "\"POSITION\":", "\"NORMAL\":", "\"TANGENT\":",
        "\"input\":", "\"output\":", "\"skin\":", "\"JOINTS_0\":", "\"WEIGHTS_0\":", "\"sampler\":", "\"node\":", "\"mesh\":"};
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
    // ---- the weights arrays of the mesh and of the node: shortened, lengthened, emptied, not finite
    for (size_t at = json.find("\"weights\":"); at != std::string::npos; at = json.find("\"weights\":", at + 1))
    {
        const size_t lb = json.find('[', at), rb = json.find(']', lb);
        const char* lists[] = {"[]", "[0]", "[1, 2, 3, 4]", "[1, 2, 3, 4, 5, 6]", "[1e39, 0, 0, 0, 0]", "[-1, -2, -3, -4, -5]"};
        for (const char* l : lists) { const std::string m = json.substr(0, lb) + l + json.substr(rb + 1); Write(var, m.data(), m.size()); Try(var); variants++; }
    }
    // ---- sparse indices out of range: every 16-bit word of the buffer's first 4 096 bytes in turn set to 42 (one past the face's last vertex) and to 65 535:
    // the sparse index views lie there, among the dense deltas
    for (size_t off = 0; off + 2 <= blob.size() && off < 4096; off += 2)
        for (uint16_t v : {(uint16_t)42, (uint16_t)65535})
        {
            std::vector<char> m = blob; std::memcpy(m.data() + off, &v, 2);
            Write(bin, m.data(), m.size()); Try(gltf); variants++;
        }
    // ---- the added buffer: truncated, and bytes overwritten (sparse indices, deltas, key times and weights among them) with a fixed-seed generator
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
