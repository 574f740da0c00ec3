"""compliancedex_amd — MI355X-native (gfx950) probabilistic-pregrasp inner loop of ComplianceDex.

Drop-in operators (same names / arguments as the reference):
  GPIS                         gpis.py:4-168
  DifferentiableRobotModel     differentiable_robot_model/robot_model.py (FK, compute_endeffector_jacobian)
  solve_ik / IKResult / DifferentiableRobotModel.inverse_kinematics / results.joint_angles_from_contacts
                               PyBullet's calculateInverseKinematics (verify_pregrasp.py:50-53): fingertips → joint
                               angles for E candidates in one launch, parity with PyBullet's solver unpinned
  solve_ik_pose / IKPoseResult / inverse_kinematics(solve_palm=True) / results.hand_pose_from_contacts
                               the same with the wrist an unknown: fingertips → joint angles and palm pose, for the
                               fingertip-space optimisers' results (the reference's writer cannot finish those)
  solve_ik_frames / IKFrameResult / inverse_kinematics(target_rot=…) / results.arm_goal_for_results
                               PyBullet's calculateInverseKinematics with a position AND an orientation
                               (verify_grasp_robot.py:48-63): link poses → joint angles with some joints held, the
                               arm's goal configuration for a stored grasp
  compute_sdf                  torchsdf/sdf.py
  ProbabilisticGraspOptimizer  optimize_pregrasp.py:614-839
  KinGraspOptimizer / SDFGraspOptimizer / GPISGraspOptimizer / KinGPISGraspOptimizer / WCKinGPISGraspOptimizer
                               optimize_pregrasp.py:121-612
  min_wrench / MinWrenchResult / solve_minimum_wrench / minimum_wrench_reward / compute_margin
                               math_utils.py:6-57 (cvxpy / cvxpylayers there): minimum-wrench contact forces of E
                               candidates in one launch with a duality-gap certificate per row, parity with SCS
                               unpinned
  force_eq_reward              optimize_pregrasp.py:73-118
  grasp_equilibrium / disturbance_report / max_payload / load_directions / gravity_loads /
  EquilibriumResult / DisturbanceReport / results.robustness_for_results
                               the PyBullet lift test of verify_pregrasp.py:82-121 asked quasi-statically: the exact
                               spring equilibrium of force_eq_reward's model for E grasps under W dead loads each in
                               one launch, with margins, normal forces, the object's displacement and a verdict per
                               grasp; no rollout, parity with PyBullet not attempted
  GPIS.pred_joint / normal_uncertainty / sample_joint / sample_normals / gpis_joint_cov / NormalUncertainty /
  shape_uncertainty_report / ShapeUncertaintyReport
                               the posterior of (f, ∇f) per query, a 4-vector Gaussian (the reference has none; its
                               compute_multinormals, gpis.py:89-111, takes normals from nested subsets of the inducing
                               points, a heuristic with no probabilistic meaning): how well a contact's normal (an
                               angular std) and the surface's position (metres) are known, draws of both, and the
                               probability that a grasp holds under disturbance_report's loads when the normals are
                               drawn.  The angular std at the packaged states is large (medians of a CPU float64
                               prototype 4 mm off the surface: 0.41 rad banana, 0.51 rad lego, 1.13 rad mug): the TPS
                               prior leaves the pointwise normal poorly determined
  farthest_point_down_sample   open3d's PointCloud.farthest_point_down_sample (optimize_pregrasp.py:904)
  cast_rays / occluded         open3d's RaycastingScene.cast_rays (concatenate_pcd.py:41-49)
  Camera / render_depth / depth_to_pointcloud / observable_pointcloud
                               get_observable_pcd.py: PyBullet's depth camera, open3d's create_from_depth_image
  GPIS.tomesh / surface_mesh   the mesh of the completed shape (train_gpis_completion.py:67-76 uses open3d's Poisson
                               reconstruction; here marching tetrahedra on the field lattice, parity unpinned), with
                               EdgeRefiner / mesh_face_vertices / to_triangle_mesh around it
  SurfaceSampler / sample_points_uniformly / sample_points_poisson_disk / GPIS.fit_mesh
                               open3d's TriangleMesh.sample_points_* (optimize_pregrasp.py:887, gpis.py:199-263):
                               area-weighted samples of a mesh's surface, parity unpinned
  knn / KnnGrid / estimate_normals / orient_normals_towards_camera_location / statistical_outlier_mask /
  remove_statistical_outlier / point_cloud_distance
                               open3d's KDTreeFlann searches, estimate_normals (concatenate_pcd.py:35-36),
                               remove_statistical_outlier and compute_point_cloud_distance: k nearest neighbours
                               of a cloud on the device, parity with open3d's covariance and eigen-solver unpinned
  HandSpheres / spheres_from_urdf / hand_collision / penetration_report
                               the whole hand as spheres on its links: penetration of the object, of itself and of
                               the floor for E candidates with the gradient in joint space (PyBullet in
                               verify_pregrasp.py and cuRobo's collision spheres in traj_gen.py there; parity unpinned)
  TrajectoryOptimizer / plan_approach / ApproachPlan / trajectory_report / seed_trajectories / interpolate / retime
                               cuRobo's MotionGen in traj_gen.py: batched CHOMP on joint-space paths from a start to
                               the grasp against the sphere model's penetration cost, a swept clearance report and
                               seed selection on the device; parity with cuRobo unpinned
  HandTerm                     that cost as a term of the joint-space optimisers' loss: optimize(..., hand_term=…)
All compute runs in libcdx.so (HIP, gfx950); importing works without a GPU, calling does not.
"""
from .gpis import GPIS, NormalUncertainty, gpis_joint_cov  # noqa: F401
from .optimizer import (EE_OFFSETS, FINGERTIP_LB, FINGERTIP_UB, WRIST_OFFSET,  # noqa: F401
                        ProbabilisticGraspOptimizer, euler_angles_to_matrix)
from .anneal import PregraspAnnealer  # noqa: F401
from .force_eq import force_eq_reward  # noqa: F401
from .optimizers import (GPISGraspOptimizer, KinGPISGraspOptimizer, KinGraspOptimizer,  # noqa: F401
                         SDFGraspOptimizer, TriangleMesh, WCKinGPISGraspOptimizer)
from .mesh import EdgeRefiner, mesh_face_vertices, refine_vertices, to_triangle_mesh  # noqa: F401
from .pointcloud import (KnnGrid, completion_arrays, estimate_normals, farthest_point_down_sample,  # noqa: F401
                         farthest_point_sample, knn, orient_normals_towards_camera_location, point_cloud_distance,
                         remove_statistical_outlier, statistical_outlier_mask)
from .raycast import (Camera, cast_rays, depth_to_pointcloud, observable_pointcloud, occluded,  # noqa: F401
                      render_depth)
from .sampling import (SurfaceSampler, sample_points_poisson_disk, sample_points_uniformly,  # noqa: F401
                       surface_sampler)
from .robot_model import DifferentiableRobotModel  # noqa: F401
from .ik import IKFrameResult, IKPoseResult, IKResult, solve_ik, solve_ik_frames, solve_ik_pose  # noqa: F401
from .dynamics import HoldingReport, holding_torques, impedance_torques  # noqa: F401
from .wrench import (MinWrenchResult, compute_margin, min_wrench, minimum_wrench_reward,  # noqa: F401
                     solve_minimum_wrench)
from .stability import (DisturbanceReport, EquilibriumResult, PayloadResult, ShapeUncertaintyReport,  # noqa: F401
                        disturbance_report, grasp_equilibrium, gravity_loads, load_directions, max_payload,
                        shape_uncertainty_report)
from .hand import HandSpheres, HandTerm, hand_collision, penetration_report, spheres_from_urdf  # noqa: F401
from .trajectory import (ApproachPlan, TrajectoryOptimizer, TrajectoryResult, interpolate, plan_approach,  # noqa: F401
                         retime, seed_trajectories, trajectory_report)
from .torchsdf import PreparedMesh, compute_sdf, compute_sdf_with_faces, index_vertices_by_faces  # noqa: F401

__version__ = "0.1.0"
