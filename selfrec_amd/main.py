"""Non-interactive launcher (the reference's main.py:10-34 asks for the model on stdin):

    python -m selfrec_amd.main XSimGCL [--conf conf/XSimGCL.yaml] [--synthetic yelp2018]
    python -m selfrec_amd.main SASRec --synthetic beauty-seq
    python -m selfrec_amd.main BERT4Rec --synthetic beauty-seq
    python -m selfrec_amd.main CL4SRec --synthetic beauty-seq
    python -m selfrec_amd.main DuoRec --synthetic beauty-seq
    python -m selfrec_amd.main SEPT --synthetic douban-book
    python -m selfrec_amd.main MHCN --synthetic douban-book

``--synthetic SHAPE`` writes a generated dataset of that shape (selfrec_amd/synth.py) to the
paths the config names, if they do not exist yet -- the reference's dataset files are not
redistributable.  A config that names a ``social.data`` file (SEPT, MHCN) gets a generated trust file the same way.
"""
import argparse
import os
import time

from . import synth
from .SELFRec import SELFRec
from .util.conf import ModelConf

MODELS = ['MF', 'LightGCN', 'XSimGCL', 'SimGCL', 'SGL', 'DirectAU', 'MixGCF', 'BUIR', 'SelfCF', 'NCL', 'UserKNN', 'ItemKNN', 'SSL4Rec', 'SASRec', 'BERT4Rec', 'CL4SRec', 'SEPT', 'MHCN', 'DuoRec', 'GRU4Rec']


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('model', choices=MODELS)
    ap.add_argument('--conf', default=None)
    ap.add_argument('--synthetic', default=None, choices=sorted(synth.SHAPES) + sorted(synth.SEQ_SHAPES))
    args = ap.parse_args(argv)
    conf = ModelConf(args.conf or f'./conf/{args.model}.yaml')
    if args.synthetic and not os.path.exists(conf['training.set']):
        os.makedirs(os.path.dirname(conf['training.set']) or '.', exist_ok=True)
        if conf['model']['type'] == 'sequential':
            if args.synthetic not in synth.SEQ_SHAPES:
                ap.error(f"a sequential model takes one of {sorted(synth.SEQ_SHAPES)}")
            train, test = synth.make_sequence_dataset(args.synthetic)
            synth.write_sequences(conf['training.set'], train)
            synth.write_sequences(conf['test.set'], test)
        else:
            if args.synthetic not in synth.SHAPES:
                ap.error(f"a graph model takes one of {sorted(synth.SHAPES)}")
            tu, ti, su, si, _, _ = synth.make_dataset(args.synthetic)
            synth.write_text(conf['training.set'], tu, ti)
            synth.write_text(conf['test.set'], su, si)
    if args.synthetic and conf.contain('social.data') and not os.path.exists(conf['social.data']):
        if args.synthetic not in synth.SHAPES:
            ap.error(f"a graph model takes one of {sorted(synth.SHAPES)}")
        os.makedirs(os.path.dirname(conf['social.data']) or '.', exist_ok=True)
        synth.write_social(conf['social.data'], synth.make_social(args.synthetic))
    t0 = time.time()
    SELFRec(conf).execute()
    print(f"Running time: {time.time() - t0:.2f} s")


if __name__ == '__main__':
    main()
