// vtk_text.hpp -- the host side of the ParaView export (host/vtk_text.cpp): sizes, argument checks, file names and XML text.
#ifndef L3K_HOST_VTK_TEXT_HPP
#define L3K_HOST_VTK_TEXT_HPP

#include "l3k.h"

#include <cstdint>
#include <string>

namespace l3k::host
{
// text bytes of the base64 stream `uint64 payload bytes || payload` (util/Base64.hpp:219-226)
inline uint64_t vtkEncodedBytes(uint64_t payload_bytes)
{
    return 4 * ((8 + payload_bytes + 2) / 3);
}
// payload bytes of a field group of `rows` rows of the field storage over n_points nodes: 1 row = 1 component, 2 or 3 rows = 3
inline uint64_t vtkGroupBytes(int rows, int64_t n_points)
{
    return uint64_t(n_points) * 8u * (rows == 1 ? 1u : 3u);
}
// cells, raw and encoded bytes of the four mesh sections; empty string, or the refusal
std::string vtkSizes(int dim, int order, int64_t n_elems, int64_t n_nodes, l3k_vtk_info& out);
// the checks of an export that need no device, in this order: nulls, rank, group sizes (vtkCheckShape), row indices, names
// (vtkCheckNames); empty string, or the refusal
std::string vtkCheckShape(int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps);
std::string vtkCheckNames(int n_groups, const char* const* names);
std::string vtkCheckGroups(int rank, int n_ranks, int n_groups, const char* const* names, const int* n_comps, const int* comp_inds,
                           int n_fields);
std::string vtkVtuFileName(const std::string& path, int rank); // <path without extension>_<rank>.vtu
std::string vtkPvtuFileName(const std::string& path);          // <path without extension>.pvtu
std::string vtkPvtuText(const std::string& path, int n_ranks, int n_groups, const char* const* names, const int* n_comps);
// everything of a .vtu in front of the appended data, the leading `_` included
std::string vtkVtuHeaderText(int64_t n_points, int64_t n_cells, const uint64_t encoded_mesh_bytes[4], int n_groups,
                             const char* const* names, const int* n_comps);
inline constexpr const char* vtk_vtu_postamble = "\n</AppendedData>\n</VTKFile>";
// creates the missing parent directories of `path`; empty string, or the refusal
std::string vtkMakeParentDirs(const std::string& path);
} // namespace l3k::host
#endif
