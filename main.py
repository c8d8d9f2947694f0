"""Entry point with the reference's command line (main.py:13-19, 60-70):

    python main.py --config train_faceDP --workspace <name> [--load_model <ckpt>]

builds the layered option object, instantiates the plugin through ``src/model/model_selector.py`` and runs fit / test with the
native trainer (dualpixelface_amd/trainer.py) instead of pytorch_lightning.  One process per GPU under torchrun.
``--synthetic N`` replaces the FaceDP loaders by N synthetic samples (no dataset is needed for a smoke run): N to train on and N // 4 to
evaluate, or all N to evaluate where the config writes a mesh per sample (reconstruct.write_ply).  Under ``use_multi`` the samples are
those of the plane scene with its neighbouring cameras (dualpixelface_amd/synthetic_multiview.py); with ``dp_render.enabled`` they are face
scenes whose dual-pixel pair is rendered on the device (dualpixelface_amd/synthetic_dp.py).
"""
import argparse
import os

import torch


def build_option(args):
    from dualpixelface_amd.config import load_option
    opt = load_option(args.config, root=os.getcwd() if os.path.isdir('config_') else None)
    opt.load_model = os.path.abspath(args.load_model) if args.load_model else None
    # workspace layout of config_manager.py:62-70
    opt.model_path = os.path.join('workspace', opt.model_name)
    opt.workspace_path = os.path.join(opt.model_path, args.workspace)
    opt.logger_path = os.path.join(opt.workspace_path, 'log')
    opt.output_path = os.path.join(opt.workspace_path, 'output')
    for d in (opt.workspace_path, opt.logger_path, opt.output_path):
        os.makedirs(d, exist_ok=True)
    return opt


def main():
    parser = argparse.ArgumentParser(description='Configuration : Dual-Pixel Face Reconstruction')
    parser.add_argument('--config', type=str, required=True, help='config to run')
    parser.add_argument('--workspace', type=str, required=True, help='workspace name')
    parser.add_argument('--load_model', type=str, help='model path to load')
    parser.add_argument('--synthetic', type=int, default=0, help='use N synthetic samples instead of the dataset on disk')
    parser.add_argument('--height', type=int, default=256)
    parser.add_argument('--width', type=int, default=384)
    parser.add_argument('--max_steps', type=int, default=None)
    args = parser.parse_args()
    opt = build_option(args)

    from dualpixelface_amd.distributed import init_from_env
    from dualpixelface_amd.trainer import Trainer
    from src.model.model_selector import model_selector
    rank, world, local = init_from_env()
    torch.manual_seed(1)                                             # seed_everything(1), main.py:24
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    model = model_selector(opt).to(device)
    trainer = Trainer(opt, opt.workspace_path, max_steps=args.max_steps, rank=rank, world_size=world)
    train_loader = val_loader = None
    if args.synthetic:
        from dualpixelface_amd.synthetic_data import synthetic_loader
        if getattr(opt, 'use_multi', False):
            from dualpixelface_amd import multiview
            from dualpixelface_amd.synthetic_multiview import synthetic_multiview_loader
            views = multiview.settings(opt).select_view

            def synthetic_loader(length, height, width, batch_size, shuffle=False, seed=0):
                return synthetic_multiview_loader(length, height, width, batch_size, views=views, shuffle=shuffle, seed=seed)
        else:
            from dualpixelface_amd import dp_render
            if dp_render.active(opt):
                from dualpixelface_amd.synthetic_dp import rendered_loader

                def synthetic_loader(length, height, width, batch_size, shuffle=False, seed=0):
                    return rendered_loader(length, height, width, batch_size, option=opt, shuffle=shuffle, seed=seed, device=device)
        train_loader = synthetic_loader(args.synthetic, args.height, args.width, opt.batch_size, shuffle=True, seed=1)
        from dualpixelface_amd import reconstruct
        held_out = args.synthetic if reconstruct.settings(opt).write_ply else max(1, args.synthetic // 4)
        val_loader = synthetic_loader(held_out, args.height, args.width, 1, seed=2)
    if opt.mode == 'train':
        trainer.fit(model, train_loader, val_loader)
    elif opt.mode == 'test':
        print(trainer.test(model, val_loader))
    else:
        raise NotImplementedError('Wrong mode !!')


if __name__ == '__main__':
    main()
