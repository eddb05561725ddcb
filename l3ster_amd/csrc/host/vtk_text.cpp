// vtk_text.cpp -- the host side of the ParaView export: sizes, argument checks, file names and the XML text of the .vtu / .pvtu
// files in the layout of the reference's post/VtkExport.hpp (pvtu_preamble / appendPvtuPointDataDef / appendPvtuPieceDataDef :102-182,
// vtu_preamble / makeDataDescription :185-189, 618-691, makeVtuFileName :498-505).  No HIP: usable without a device.
//
// One deviation, on purpose: the reference's .pvtu loop (:117-143) labels a SECOND vector group as `Scalars` when no scalar group
// precedes it, while its .vtu names the first 1-component group.  Here both files follow one rule: Scalars = the first 1-component
// group (if any), Vectors = the first 3-component group (if any), Scalars in front of Vectors.
#include "host/vtk_text.hpp"

#include <cstdio>
#include <cstring>
#include <filesystem>
#include <system_error>

namespace l3k::dev
{
void setError(const char* fmt, ...);
}

namespace l3k::host
{
namespace
{
constexpr uint64_t uint32_limit = 0xffffffffull; // what a UInt32 array of the format can hold

int nComponents(int rows)
{
    return rows == 1 ? 1 : 3;
}
// PointData attributes: ` Scalars="first 1-component group"` ` Vectors="first 3-component group"`
void appendActiveArrays(std::string& s, int n_groups, const char* const* names, const int* n_comps)
{
    int scalar = -1, vector = -1;
    for (int g = 0; g < n_groups; ++g)
    {
        if (n_comps[g] == 1 && scalar < 0)
            scalar = g;
        if (n_comps[g] != 1 && vector < 0)
            vector = g;
    }
    if (scalar >= 0)
        s.append(" Scalars=\"").append(names[scalar]).append("\"");
    if (vector >= 0)
        s.append(" Vectors=\"").append(names[vector]).append("\"");
}
} // namespace

std::string vtkSizes(int dim, int order, int64_t n_elems, int64_t n_nodes, l3k_vtk_info& out)
{
    if ((dim != 2 && dim != 3) || order < 1 || order > 8 || n_elems < 0 || n_nodes < 0)
        return "l3k_vtk_sizes: dim must be 2 or 3, order in [1, 8], counts non-negative";
    uint64_t per_elem = 1; // sub-cells of an element
    for (int d = 0; d < dim; ++d)
        per_elem *= uint64_t(order);
    const uint64_t corners = dim == 2 ? 4 : 8;
    // n_elems < 2^63 and per_elem * corners <= 4096: the comparison is made without forming the product
    const bool conn_fits = uint64_t(n_elems) <= uint32_limit / (per_elem * corners);
    if (uint64_t(n_nodes) > uint32_limit || !conn_fits)
    {
        const long double conn = static_cast< long double >(n_elems) * static_cast< long double >(per_elem * corners);
        char              buf[256];
        std::snprintf(buf, sizeof buf,
                      "l3k_vtk_sizes: %lld local nodes and %.0Lf connectivity entries: the UInt32 arrays of the format hold at most "
                      "4294967295 of either",
                      (long long)n_nodes, conn);
        return buf;
    }
    out              = l3k_vtk_info{};
    out.dim          = dim;
    out.order        = order;
    out.n_points     = n_nodes;
    out.n_cells      = int64_t(uint64_t(n_elems) * per_elem);
    out.n_conn       = out.n_cells * int64_t(corners);
    out.raw_bytes[0] = uint64_t(n_nodes) * 24u;
    out.raw_bytes[1] = uint64_t(out.n_conn) * 4u;
    out.raw_bytes[2] = uint64_t(out.n_cells) * 4u;
    out.raw_bytes[3] = uint64_t(out.n_cells);
    for (int k = 0; k < 4; ++k)
        out.encoded_bytes[k] = vtkEncodedBytes(out.raw_bytes[k]);
    return {};
}

std::string vtkCheckShape(int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps)
{
    if (n_groups < 0 || (n_groups > 0 && (!names || !n_comps)))
        return "null or negative argument";
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return "rank " + std::to_string(rank) + " outside [0, n_ranks = " + std::to_string(n_ranks) + ")";
    for (int g = 0; g < n_groups; ++g)
        if (n_comps[g] < 1 || n_comps[g] > 3)
            return "Field groupings must have size 1 (scalar), 2 (2D), or 3 (3D)"; // VtkExport.hpp:454-455
    return {};
}
std::string vtkCheckNames(int n_groups, const char* const* names)
{
    for (int g = 0; g < n_groups; ++g)
        if (!names[g] || !names[g][0] || std::strpbrk(names[g], "\"<>&"))
            return "name of field group " + std::to_string(g) + " is empty or contains one of \" < > &: the file would not be well-formed";
    return {};
}
std::string vtkCheckGroups(int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps, const int* comp_inds,
                           int n_fields)
{
    if (n_fields < 0 || (n_groups > 0 && !comp_inds))
        return "null or negative argument";
    if (std::string err = vtkCheckShape(rank, n_ranks, n_groups, names, n_comps); !err.empty())
        return err;
    for (int g = 0, at = 0; g < n_groups; ++g)
        for (int c = 0; c < n_comps[g]; ++c, ++at)
            if (comp_inds[at] < 0 || comp_inds[at] >= n_fields)
                return "Out of bounds index"; // :536-537
    return vtkCheckNames(n_groups, names);
}

std::string vtkVtuFileName(const std::string& path, int rank)
{
    return std::filesystem::path{path}.replace_extension().string() + "_" + std::to_string(rank) + ".vtu";
}
std::string vtkPvtuFileName(const std::string& path)
{
    return std::filesystem::path{path}.replace_extension("pvtu").string();
}

std::string vtkPvtuText(const std::string& path, int n_ranks, int n_groups, const char* const* names, const int* n_comps)
{
    std::string s = "<?xml version=\"1.0\"?>\n"
                    "<VTKFile type=\"PUnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\">\n"
                    "<PUnstructuredGrid GhostLevel=\"0\">\n"
                    "<PPoints>\n"
                    "  <PDataArray type=\"Float64\" Name=\"Position\" NumberOfComponents=\"3\"/>\n"
                    "</PPoints>\n"
                    "<PCells>\n"
                    "  <PDataArray type=\"UInt32\" Name=\"connectivity\" NumberOfComponents=\"1\"/>\n"
                    "  <PDataArray type=\"UInt32\" Name=\"offsets\" NumberOfComponents=\"1\"/>\n"
                    "  <PDataArray type=\"UInt8\" Name=\"types\" NumberOfComponents=\"1\"/>\n"
                    "</PCells>\n"
                    "<PPointData";
    appendActiveArrays(s, n_groups, names, n_comps);
    s += ">\n";
    for (int g = 0; g < n_groups; ++g)
        s.append("  <PDataArray type=\"Float64\" Name=\"")
            .append(names[g])
            .append("\" NumberOfComponents=\"")
            .append(std::to_string(nComponents(n_comps[g])))
            .append("\"/>\n");
    s += "</PPointData>\n<PCellData>\n</PCellData>\n";
    const std::string stem = std::filesystem::path{path}.stem().string(); // no directory: the pieces lie beside the .pvtu
    for (int r = 0; r < n_ranks; ++r)
        s.append("<Piece Source=\"").append(stem).append("_").append(std::to_string(r)).append(".vtu\"/>\n");
    s += "</PUnstructuredGrid>\n</VTKFile>";
    return s;
}

std::string vtkVtuHeaderText(int64_t n_points, int64_t n_cells, const uint64_t encoded_mesh_bytes[4], int n_groups,
                             const char* const* names, const int* n_comps)
{
    std::string s = "<?xml version=\"1.0\"?>\n"
                    "<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" header_type=\"UInt64\">\n"
                    "<UnstructuredGrid>\n";
    uint64_t   offset = 0;
    const auto array  = [&](const char* type, const char* name, int n_components, uint64_t encoded_bytes) {
        s.append("  <DataArray type=\"")
            .append(type)
            .append("\" Name=\"")
            .append(name)
            .append("\" NumberOfComponents=\"")
            .append(std::to_string(n_components))
            .append("\" format=\"appended\" offset=\"")
            .append(std::to_string(offset))
            .append("\">\n  </DataArray>\n");
        offset += encoded_bytes;
    };
    s.append("<Piece NumberOfPoints=\"").append(std::to_string(n_points)).append("\" NumberOfCells=\"").append(std::to_string(n_cells));
    s += "\">\n<Points>\n";
    array("Float64", "Position", 3, encoded_mesh_bytes[0]);
    s += "</Points>\n<Cells>\n";
    array("UInt32", "connectivity", 1, encoded_mesh_bytes[1]);
    array("UInt32", "offsets", 1, encoded_mesh_bytes[2]);
    array("UInt8", "types", 1, encoded_mesh_bytes[3]);
    s += "</Cells>\n<PointData";
    appendActiveArrays(s, n_groups, names, n_comps);
    s += ">\n";
    for (int g = 0; g < n_groups; ++g)
        array("Float64", names[g], nComponents(n_comps[g]), vtkEncodedBytes(vtkGroupBytes(n_comps[g], n_points)));
    s += "</PointData>\n<CellData>\n</CellData>\n</Piece>\n</UnstructuredGrid>\n<AppendedData encoding=\"base64\">\n  _";
    return s;
}

std::string vtkMakeParentDirs(const std::string& path)
{
    std::error_code ec;
    const auto      parent = std::filesystem::absolute(path, ec).parent_path(); // VtkExport.hpp:544
    if (!ec && !parent.empty())
        std::filesystem::create_directories(parent, ec);
    if (ec || !std::filesystem::is_directory(parent, ec))
        return "cannot create the directory " + parent.string() + (ec ? ": " + ec.message() : std::string{});
    return {};
}
} // namespace l3k::host

namespace
{
// the text into the caller's buffer: *needed = its length (without a terminator); copied only if it fits
int giveText(const char* who, const std::string& text, char* buf, size_t capacity, size_t* needed)
{
    if (needed)
        *needed = text.size();
    if (!buf)
        return 0; // the size query
    if (capacity < text.size())
    {
        l3k::dev::setError("%s: the text has %zu bytes, the buffer %zu", who, text.size(), capacity);
        return -1;
    }
    std::memcpy(buf, text.data(), text.size());
    return 0;
}
} // namespace

extern "C" {

int l3k_vtk_sizes(int dim, int order, int64_t n_elems, int64_t n_nodes, l3k_vtk_info* out)
{
    if (!out)
    {
        l3k::dev::setError("l3k_vtk_sizes: null argument");
        return -1;
    }
    l3k_vtk_info      info{};
    const std::string err = l3k::host::vtkSizes(dim, order, n_elems, n_nodes, info);
    if (!err.empty())
    {
        l3k::dev::setError("%s", err.c_str());
        return -1;
    }
    *out = info;
    return 0;
}

int l3k_vtk_pvtu_text(const char* path, int n_ranks, int n_groups, const char* const* names, const int* n_comps, char* buf,
                      size_t capacity, size_t* needed)
{
    if (!path || (!buf && !needed))
    {
        l3k::dev::setError("l3k_vtk_pvtu_text: null argument");
        return -1;
    }
    std::string err = l3k::host::vtkCheckShape(0, n_ranks, n_groups, names, n_comps);
    if (err.empty())
        err = l3k::host::vtkCheckNames(n_groups, names);
    if (!err.empty())
    {
        l3k::dev::setError("l3k_vtk_pvtu_text: %s", err.c_str());
        return -1;
    }
    return giveText("l3k_vtk_pvtu_text", l3k::host::vtkPvtuText(path, n_ranks, n_groups, names, n_comps), buf, capacity, needed);
}

int l3k_vtk_vtu_header_text(int64_t n_points, int64_t n_cells, const uint64_t* encoded_mesh_bytes, int n_groups, const char* const* names,
                            const int* n_comps, char* buf, size_t capacity, size_t* needed)
{
    if (!encoded_mesh_bytes || (!buf && !needed) || n_points < 0 || n_cells < 0)
    {
        l3k::dev::setError("l3k_vtk_vtu_header_text: null or negative argument");
        return -1;
    }
    std::string err = l3k::host::vtkCheckShape(0, 1, n_groups, names, n_comps);
    if (err.empty())
        err = l3k::host::vtkCheckNames(n_groups, names);
    if (!err.empty())
    {
        l3k::dev::setError("l3k_vtk_vtu_header_text: %s", err.c_str());
        return -1;
    }
    return giveText("l3k_vtk_vtu_header_text", l3k::host::vtkVtuHeaderText(n_points, n_cells, encoded_mesh_bytes, n_groups, names, n_comps),
                    buf, capacity, needed);
}

} // extern "C"
