"""Worker of tests/test_gpu_joint_finetune.py::test_one_rank_distributed_joint_step_bit_exact: a
fresh process with a ONE-rank RCCL group (torchrun-style env), in which the joint FinetuneTrainer
step with distributed=True (both flat gradients all-reduced) runs beside the distributed=False
one.  Writes both runs' losses, gradients and parameters to argv[1]."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build():
    from image_denoising_amd import UNet
    from image_denoising_amd.adapter import DenoiserWithAdapter

    torch.manual_seed(0)
    base = UNet(in_nc=1, out_nc=1, n_feature=48)
    torch.manual_seed(1)
    return DenoiserWithAdapter(base, 1, 16, freeze_base=False, use_no_grad_for_base=False).to("cuda")


def run(distributed):
    from image_denoising_amd.finetune import FinetuneTrainer

    model = build()
    tr = FinetuneTrainer(model, lr=1e-4, lambda_grad=0.1, distributed=distributed)
    assert tr.distributed == distributed and tr.joint
    g = torch.Generator().manual_seed(9)
    losses = []
    for _ in range(2):
        clean = torch.rand(2, 1, 32, 32, generator=g)
        noisy = clean + 0.1 * torch.randn(2, 1, 32, 32, generator=g)
        losses.append(tr.train_step(clean.cuda(), noisy.cuda()))
    torch.cuda.synchronize()
    return dict(losses=torch.stack(losses).cpu().numpy(), grad=tr.grad.cpu().numpy(),
                base_grad=tr.base_grad.cpu().numpy(),
                adapter=model.adapter.flat_params.detach().cpu().numpy(),
                base=model.base.flat_params.detach().cpu().numpy())


def main():
    from image_denoising_amd import dist as dp

    world, _, _ = dp.init_from_env("nccl", force=True)
    assert world == 1 and dp.is_initialized()
    a, b = run(True), run(False)
    np.savez(sys.argv[1], backend=np.array(dist.get_backend()),
             **{k: v for k, v in a.items()}, **{k + "_local": v for k, v in b.items()})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
