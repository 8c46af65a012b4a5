"""torch restatement of tests/mano_ref.py with ``dtype`` and ``device`` parameters -- test infrastructure.

Written from that file's steps, one for one, in differentiable torch operations: autograd through it is the reference for the MANO
layer's backward pass (dvq_mano_backward).  In float64 on the CPU it is the reference; in float32 on the CPU it is the source of
``e32``, the error a plain fp32 evaluation of the same gradient makes; in float32 on the GPU it is what a user without the fused
backward would write (tools/mano_backward_rate.py).  ``1 - cos a`` is ``2 sin^2(a/2)``, as in mano_ref.rodrigues.  Feed it
``mano_ref.device_arrays(arrays)``: the model as the device holds it."""
import numpy as np
import torch

NV, NJ, NB, NP = 778, 16, 10, 45


class ManoTorch:
    def __init__(self, arrays, flat_hand_mean=True, dtype=torch.float64, device="cpu"):
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype, device=device)
        self.dtype, self.device = dtype, device
        self.vt = t(arrays["v_template"])
        self.sd = t(np.asarray(arrays["shapedirs"], np.float64)[:, :, :NB].reshape(NV * 3, NB))
        self.pd = t(np.asarray(arrays["posedirs"], np.float64).reshape(NV * 3, 9 * (NJ - 1)))
        self.jr, self.w = t(arrays["J_regressor"]), t(arrays["weights"])
        self.comps = t(np.asarray(arrays["hands_components"], np.float64)[:NP])
        mean = np.zeros(NP) if flat_hand_mean else np.asarray(arrays["hands_mean"], np.float64)
        self.mean = t(np.concatenate([np.zeros(3), mean]))
        self.parents = [int(p) for p in np.asarray(arrays["parents"]).reshape(-1)]

    def rodrigues(self, r):
        """[..., 3] -> [..., 3, 3], angle = ||r + 1e-8||."""
        e = r + 1e-8
        angle = torch.sqrt((e * e).sum(-1))
        d = r / angle[..., None]
        z = torch.zeros_like(angle)
        K = torch.stack([z, -d[..., 2], d[..., 1], d[..., 2], z, -d[..., 0], -d[..., 1], d[..., 0], z], dim=-1).reshape(r.shape[:-1] + (3, 3))
        s = torch.sin(angle)[..., None, None]
        c1 = (2.0 * torch.sin(0.5 * angle) ** 2)[..., None, None]
        return torch.eye(3, dtype=r.dtype, device=r.device) + s * K + c1 * (K @ K)

    def __call__(self, betas, hand_pose, global_orient=None, transl=None):
        """-> (verts [B,778,3], joints [B,16,3])."""
        B = betas.shape[0]
        go = torch.zeros(B, 3, dtype=self.dtype, device=self.device) if global_orient is None else global_orient
        tr = torch.zeros(B, 3, dtype=self.dtype, device=self.device) if transl is None else transl
        # 1. PCA pose -> axis-angle, plus the mean pose
        full_pose = torch.cat([go, hand_pose @ self.comps], dim=1) + self.mean
        # 2. shape blendshapes and the joints regressed from the shaped mesh
        v_shaped = self.vt[None] + (betas @ self.sd.T).reshape(B, NV, 3)
        J = torch.einsum("jv,bvk->bjk", self.jr, v_shaped)
        # 3. joint rotations
        R = self.rodrigues(full_pose.reshape(B, NJ, 3))
        # 4. pose blendshapes
        pose_feature = (R[:, 1:] - torch.eye(3, dtype=self.dtype, device=self.device)).reshape(B, 9 * (NJ - 1))
        v_posed = v_shaped + (pose_feature @ self.pd.T).reshape(B, NV, 3)
        # 5. kinematic chain
        Gr, Gt = [None] * NJ, [None] * NJ
        for j in range(NJ):
            p = self.parents[j]
            if p < 0:
                Gr[j], Gt[j] = R[:, j], J[:, j]
            else:
                Gr[j] = Gr[p] @ R[:, j]
                Gt[j] = (Gr[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p]
        Gr, Gt = torch.stack(Gr, dim=1), torch.stack(Gt, dim=1)
        At = Gt - (Gr @ J[..., None])[..., 0]
        # 6. skinning
        Tr = torch.einsum("vj,bjik->bvik", self.w, Gr)
        Tt = torch.einsum("vj,bji->bvi", self.w, At)
        verts = (Tr @ v_posed[..., None])[..., 0] + Tt + tr[:, None]
        joints = Gt + tr[:, None]
        return verts, joints

    def vjp(self, betas, hand_pose, global_orient=None, transl=None, grad_verts=None, grad_joints=None):
        """Gradients of <verts, grad_verts> + <joints, grad_joints> -> (g_betas, g_pose, g_global_orient, g_transl) as float64 numpy
        arrays ([B,3] zeros for an input that was not given)."""
        cv = lambda x: None if x is None else torch.as_tensor(np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64),
                                                              dtype=self.dtype, device=self.device)
        ins = [cv(x) for x in (betas, hand_pose, global_orient, transl)]
        B = ins[0].shape[0]
        for i in (2, 3):
            if ins[i] is None:
                ins[i] = torch.zeros(B, 3, dtype=self.dtype, device=self.device)
        ins = [x.clone().requires_grad_(True) for x in ins]
        verts, joints = self(*ins)
        loss = 0.0
        if grad_verts is not None:
            loss = loss + (verts * cv(grad_verts)).sum()
        if grad_joints is not None:
            loss = loss + (joints * cv(grad_joints)).sum()
        grads = torch.autograd.grad(loss, ins, allow_unused=True)
        return tuple(np.zeros(tuple(x.shape)) if g is None else g.detach().cpu().double().numpy() for g, x in zip(grads, ins))
