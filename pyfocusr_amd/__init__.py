"""pyfocusr_amd — MI355X-native spectral-embedding hot path of pyfocusr.

Same public names as the reference package (`/root/reference/pyfocusr/__init__.py:1-5`):
`Focusr`, `Graph`, `recursive_eig`, `vtk_functions`; plus `eigsort` and the
device binding.  Importing the package does not touch the GPU; the first device
call loads `csrc/libpyfocusr_hip.so` and fails loudly if it (or an MI355X) is
missing — there is no CPU fallback.
"""
from . import vtk_functions
from .assignment import euclidean_assignment
from .correspondence import closest_points_on_embedded_surface, interpolate_on_surface, transfer_point_data
from .components import (ComponentStats, component_boxes, connected_components, fill_holes, keep_largest_components,
                         largest_component_per_label, remove_small_components)
from .curvature import (curvature_on_mesh, curvedness, discrete_curvatures, principal_curvatures, shape_index)
from .eigsort import eigsort
from .focusr import *  # noqa: F401,F403
from .graph import *  # noqa: F401,F403
from .functional_maps import (fast_zoomout_correspondences, functional_map_from_p2p, p2p_from_functional_map,
                              soft_p2p_from_functional_map, zoomout_correspondences, zoomout_refine)
from .map_quality import (conformal_distortion, distortion_on_mesh, isometric_distortion, map_distortion,
                          symmetric_dirichlet)
from .distance_transform import (close_mask, dilate_mask, distance_transform, erode_mask, mask_offset_surface, nearest_feature,
                                 open_mask, propagate_labels, signed_distance_of_mask)
from .isosurface import isosurface, mask_to_mesh, offset_surface, signed_distance_volume, voxel_remesh
from .neighbours import inverse_distance_average, k_nearest_neighbours
from .laplace_beltrami import cotangent_laplacian, laplace_beltrami_spectrum, mean_curvature, mean_curvature_normals
from .sampling import farthest_point_sampling, voronoi_masses
from .ray_casting import (hit_points, ray_crossings, ray_mesh_intersections, thickness_along_normals,
                          vertex_normals)
from .remesh import lift_point_map, prolong_from_clusters, resample_mesh, restrict_to_clusters
from .shape_model import ShapeModel, build_shape_model, generalized_procrustes, population_from_template
from .smoothing import MeshSmoother, smooth_mask_mesh, smooth_mesh, smooth_point_data
from .spectral_descriptors import (descriptor_coefficients, descriptor_correspondences, functional_map_from_descriptors,
                                   heat_kernel_signature, signature_on_mesh, spectral_descriptors, wave_kernel_signature)
from .surface_distance import (point_to_surface_distances, points_inside, signed_distances_on_mesh,
                               signed_point_to_surface_distances, summarize_distances, summarize_signed_distances,
                               surface_distance_metrics, winding_numbers)
from .test import get_all_pairwise_surface_errors
from .topology import extract_patches, is_consistently_oriented, mesh_topology, orient_faces
from .vtk_functions import PolyMesh, read_vtk_mesh, write_vtk_mesh

__version__ = "0.1.0"
